// sbm_pgo.hip -- the pose-graph optimiser: the reference's runOptimize / runOptimizeRobust (Optimizer.cpp, HyperGraph.cpp,
// GraphEdge.cpp, GraphVertex.cpp, g2o/SE3Gradient.cpp, getConnectedGraph of Mapper.cpp) with the Levenberg-Marquardt iteration
// on the device. include/sbm.h states the arithmetic; tests/pgo_cases.py restates it in numpy. Everything is fp64, nothing is
// contracted (the Makefile says so too), and there is no atomic anywhere: every sum has one owner and a fixed order.
//   linearise  one lane per edge: error, chi2, both Jacobians, Ji^T O Ji, Jj^T O Jj, Ji^T O Jj, Ji^T(-Oe), Jj^T(-Oe)
//   assemble   one lane per free vertex (its diagonal block and b, incident edges in edge order) and per off-diagonal slot
//   solve      (twice: b, then the residual of the first x taken in twice the working precision, against the same factors)
//              block Thomas on the runs (16 lanes per run, one right-hand column each), the Schur complement on the junctions,
//              a dense block Cholesky of it (one launch per block column), two triangular solves, back-substitution
//   update     oplus per free vertex and the per-vertex terms of scaleLambda's sum
// The partition into runs and junctions (PgoPlan) and getConnectedGraph are host code and need no device: sbm_pgo_plan.hip has
// them, sbm_pgo.h what the two files share (the rigid-transform arithmetic among it).
#include <math.h>

#include <cmath>
#include <algorithm>
#include <map>
#include <new>
#include <vector>

#include "sbm_handle.h"
#include "sbm_pgo.h"

#pragma clang fp contract(off)

namespace sbm {

constexpr int kPgoRunLanes = 16;         // lanes per run: 13 right-hand columns, 3 idle
constexpr int kPgoCols = 13;             // b, the 6 columns towards the left junction, the 6 towards the right one

enum PgoStage { kPgLinearise, kPgAssemble, kPgSolve, kPgUpdate, kPgTotal, kPgStageCount };
enum PgoMark { kPgBegin, kPgLinearised, kPgAssembled, kPgSolved, kPgEnd, kPgMarkCount };
static const char* const kPgoNames[] = {"pgo_linearise", "pgo_assemble", "pgo_solve", "pgo_update", "pgo_total"};
StageTable pgo_stages() { return stage_table<kPgStageCount, kPgMarkCount>(kPgoNames); }

// ---- 6x6 arithmetic, every sum left to right (the 3x3 products and Rt are in sbm_pgo.h) --------------------------------------------
// Eigen's Quaternion(Matrix3), both branches; q = (x, y, z, w)
__device__ static inline void quat_from_matrix(const double m[3][3], double q[4]) {
  double t = (m[0][0] + m[1][1]) + m[2][2];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[2][1] - m[1][2]) * t;
    q[1] = (m[0][2] - m[2][0]) * t;
    q[2] = (m[1][0] - m[0][1]) * t;
  } else {
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > m[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[k][j] - m[j][k]) * t;
    q[j] = (m[j][i] + m[i][j]) * t;
    q[k] = (m[k][i] + m[i][k]) * t;
  }
}

// Edge::computeError: delta = (Z^-1 * Xi^-1) * Xj
__device__ static void edge_error(const Rt& Z, const Rt& Xi, const Rt& Xj, double e[6]) {
  const Rt d = compose(compose(inverse(Z), inverse(Xi)), Xj);
  double q[4];
  quat_from_matrix(d.R, q);
  const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int i = 0; i < 4; i++) q[i] = q[i] / n;
  const bool neg = q[3] < 0;
  for (int i = 0; i < 3; i++) {
    e[i] = d.t[i];
    e[3 + i] = neg ? -q[i] : q[i];
  }
}

__device__ static inline void mat6_vec(const double* M, const double* v, double* o) {   // M row-major
  for (int i = 0; i < 6; i++) {
    double s = M[6 * i] * v[0];
    for (int j = 1; j < 6; j++) s = s + M[6 * i + j] * v[j];
    o[i] = s;
  }
}
__device__ static inline void matT_vec(const double* M, const double* v, double* o) {
  for (int i = 0; i < 6; i++) {
    double s = M[i] * v[0];
    for (int r = 1; r < 6; r++) s = s + M[6 * r + i] * v[r];
    o[i] = s;
  }
}
__device__ static inline void matT_mat(const double* A, const double* B, double* C) {   // A^T B
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double s = A[i] * B[j];
      for (int r = 1; r < 6; r++) s = s + A[6 * r + i] * B[6 * r + j];
      C[6 * i + j] = s;
    }
}
__device__ static inline void mat_mat(const double* A, const double* B, double* C) {
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double s = A[6 * i] * B[j];
      for (int r = 1; r < 6; r++) s = s + A[6 * i + r] * B[6 * r + j];
      C[6 * i + j] = s;
    }
}

// dq_dR (3 x 9) times the 9 x 3 matrix whose column c is the column-major 3 x 3 product L * S[c]
__device__ static void dq_times(const double dq[3][9], const double L[3][3], const double S[3][3][3], double out[3][3]) {
  double M[9][3];
  for (int c = 0; c < 3; c++) {
    double P[3][3];
    mul33(L, S[c], P);
    for (int cc = 0; cc < 3; cc++)
      for (int r = 0; r < 3; r++) M[r + 3 * cc][c] = P[r][cc];
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = dq[i][0] * M[0][j];
      for (int k = 1; k < 9; k++) s = s + dq[i][k] * M[k][j];
      out[i][j] = s;
    }
}
__device__ static void skew2(const double R[3][3], bool transposed, double S[3][3][3]) {
  const double sg = transposed ? 1.0 : -1.0;
  for (int a = 0; a < 3; a++)
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) S[a][i][j] = 0.0;
  for (int j = 0; j < 3; j++) {
    const double r0 = 2 * R[0][j], r1 = 2 * R[1][j], r2 = 2 * R[2][j];
    S[0][1][j] = sg * r2;  S[0][2][j] = -sg * r1;
    S[1][0][j] = -sg * r2; S[1][2][j] = sg * r0;
    S[2][0][j] = sg * r1;  S[2][1][j] = -sg * r0;
  }
}

// computeEdgeSE3Gradient as written, the singular form of dq/dR at a 180 degree error included
__device__ static void edge_jacobians(const Rt& Z, const Rt& Xi, const Rt& Xj, double* Ji, double* Jj) {
  const Rt A = inverse(Z), B = compose(inverse(Xi), Xj), E = compose(A, B);
  const double tr = (E.R[0][0] + E.R[1][1]) + E.R[2][2];
  const double S = sqrt(tr + 1.0) * 2;
  const double qw = S * .25;
  const double a1 = 1 / pow(qw, 3.0);
  const double a2 = -0.03125 * (E.R[2][1] - E.R[1][2]) * a1;
  const double a3 = 1 / qw;
  const double a4 = 0.25 * a3, a5 = -0.25 * a3;
  const double a6 = 0.03125 * (E.R[2][0] - E.R[0][2]) * a1;
  const double a7 = -0.03125 * (E.R[1][0] - E.R[0][1]) * a1;
  const double dq[3][9] = {{a2, 0, 0, 0, a2, a4, 0, a5, a2}, {a6, 0, a5, 0, a6, 0, a4, 0, a6}, {a7, a4, 0, a5, a7, 0, 0, 0, a7}};
  for (int i = 0; i < 36; i++) Ji[i] = Jj[i] = 0.0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      Ji[6 * i + j] = -A.R[i][j];
      Jj[6 * i + j] = E.R[i][j];
    }
  const double x = 2 * B.t[0], y = 2 * B.t[1], z = 2 * B.t[2];
  const double Sk[3][3] = {{0.0, -z, y}, {z, 0.0, -x}, {-y, x, 0.0}};
  double P[3][3], S3[3][3][3];
  mul33(A.R, Sk, P);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Ji[6 * i + 3 + j] = P[i][j];
  skew2(B.R, true, S3);
  dq_times(dq, A.R, S3, P);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Ji[6 * (3 + i) + 3 + j] = P[i][j];
  const double I3[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  skew2(I3, false, S3);
  dq_times(dq, E.R, S3, P);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Jj[6 * (3 + i) + 3 + j] = P[i][j];
}

// ---- per-edge records -----------------------------------------------------------------------------------------------------------
// One record of 200 doubles per edge: e 6, chi2 1, pad 1, Ji 36, Jj 36, mii 36, mjj 36, mij 36, bi 6, bj 6 (row-major blocks).
constexpr int kRecE = 0, kRecChi = 6, kRecJi = 8, kRecJj = 44, kRecMii = 80, kRecMjj = 116, kRecMij = 152, kRecBi = 188,
              kRecBj = 194, kRec = 200;

__global__ __launch_bounds__(64) void pgo_linearise_kernel(int ne, const int* __restrict__ vi, const int* __restrict__ vj,
                                                            const int* __restrict__ hidx, const double* __restrict__ poses,
                                                            const double* __restrict__ meas, const double* __restrict__ info,
                                                            int errors_only, double* __restrict__ rec, double* __restrict__ chi,
                                                            double* __restrict__ scal) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= ne) return;
  const Rt Z = load_rt(meas + 12 * (size_t)k), Xi = load_rt(poses + 12 * (size_t)vi[k]), Xj = load_rt(poses + 12 * (size_t)vj[k]);
  const double* O = info + 36 * (size_t)k;
  double* r = rec + (size_t)kRec * k;
  double e[6], Oe[6];
  edge_error(Z, Xi, Xj, e);
  mat6_vec(O, e, Oe);
  double c = e[0] * Oe[0];
  for (int i = 1; i < 6; i++) c = c + e[i] * Oe[i];
  chi[k] = c;
  if (errors_only) return;   // computeActiveErrors: the records of the last linearisation stay as they are
  for (int i = 0; i < 6; i++) r[kRecE + i] = e[i];
  r[kRecChi] = c;
  double Ji[36], Jj[36], JO[36], m[36], we[6], b[6];
  edge_jacobians(Z, Xi, Xj, Ji, Jj);
  for (int i = 0; i < 36; i++) { r[kRecJi + i] = Ji[i]; r[kRecJj + i] = Jj[i]; }
  for (int i = 0; i < 6; i++) we[i] = -Oe[i];
  matT_vec(Ji, we, b);
  for (int i = 0; i < 6; i++) r[kRecBi + i] = b[i];
  matT_vec(Jj, we, b);
  for (int i = 0; i < 6; i++) r[kRecBj + i] = b[i];
  double max_diag = 0.0;   // Edge::constructQuadraticForm resets it for every edge: the last edge's value is what stays
  matT_mat(Ji, O, JO);
  mat_mat(JO, Ji, m);
  for (int i = 0; i < 36; i++) r[kRecMii + i] = m[i];
  if (hidx[vi[k]] >= 0)
    for (int i = 0; i < 6; i++) max_diag = fabs(m[7 * i]) > max_diag ? fabs(m[7 * i]) : max_diag;
  mat_mat(JO, Jj, m);
  for (int i = 0; i < 36; i++) r[kRecMij + i] = m[i];
  matT_mat(Jj, O, JO);
  mat_mat(JO, Jj, m);
  for (int i = 0; i < 36; i++) r[kRecMjj + i] = m[i];
  if (hidx[vj[k]] >= 0)
    for (int i = 0; i < 6; i++) max_diag = fabs(m[7 * i]) > max_diag ? fabs(m[7 * i]) : max_diag;
  if (k == ne - 1) scal[2] = max_diag;
}

// Fixed-shape sum of n doubles into *dst: 256 lanes take strided partial sums in index order, then a binary tree.
__global__ __launch_bounds__(256) void pgo_reduce_kernel(const double* __restrict__ src, int n, double* __restrict__ dst) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s = s + src[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *dst = part[0];
}

// Lanes [0, nfree): D[h] (the diagonal block as the triplets place it: entry (j, i) receives m(i, j)) and b[h] from the
// incidence list, in edge order. Lanes [nfree, nfree + nslots): the lower off-diagonal block of one vertex pair, the sum of its
// edges' m_ij^T (to holds the larger index) or m_ij (mirrored from the upper triangle, SYMMETRIC only).
__global__ __launch_bounds__(64) void pgo_assemble_kernel(int nfree, int nslots, const int* __restrict__ inc_ptr,
                                                           const int* __restrict__ inc, const int* __restrict__ slot_ptr,
                                                           const int* __restrict__ slot_edge, const double* __restrict__ rec,
                                                           double* __restrict__ D, double* __restrict__ bv, double* __restrict__ Eoff) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t < nfree) {
    double acc[36], b[6];
    for (int i = 0; i < 36; i++) acc[i] = 0.0;
    for (int i = 0; i < 6; i++) b[i] = 0.0;
    for (int p = inc_ptr[t]; p < inc_ptr[t + 1]; p++) {
      const int code = inc[p];                     // edge * 2 + end
      const double* r = rec + (size_t)kRec * (code >> 1);
      const double* m = r + ((code & 1) ? kRecMjj : kRecMii);
      const double* bb = r + ((code & 1) ? kRecBj : kRecBi);
      for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) acc[6 * j + i] = acc[6 * j + i] + m[6 * i + j];
      for (int i = 0; i < 6; i++) b[i] = b[i] + bb[i];
    }
    for (int i = 0; i < 36; i++) D[36 * (size_t)t + i] = acc[i];
    for (int i = 0; i < 6; i++) bv[6 * (size_t)t + i] = b[i];
  } else if (t < nfree + nslots) {
    const int s = t - nfree;
    double acc[36];
    for (int i = 0; i < 36; i++) acc[i] = 0.0;
    for (int p = slot_ptr[s]; p < slot_ptr[s + 1]; p++) {
      const int code = slot_edge[p];               // edge * 2 + (1 when the block goes in as m, 0 as m^T)
      const double* m = rec + (size_t)kRec * (code >> 1) + kRecMij;
      if (code & 1)
        for (int i = 0; i < 36; i++) acc[i] = acc[i] + m[i];
      else
        for (int i = 0; i < 6; i++)
          for (int j = 0; j < 6; j++) acc[6 * j + i] = acc[6 * j + i] + m[6 * i + j];
    }
    for (int i = 0; i < 36; i++) Eoff[36 * (size_t)s + i] = acc[i];
  }
}

// ---- 6x6 factor helpers ---------------------------------------------------------------------------------------------------------
// G lower with G G^T = A (A's lower triangle is read); the upper triangle of G is set to 0.
__device__ static inline void chol6(const double* A, double* G) {
  for (int j = 0; j < 6; j++) {
    double d = A[7 * j];
    for (int k = 0; k < j; k++) d = d - G[6 * j + k] * G[6 * j + k];
    d = sqrt(d);
    G[7 * j] = d;
    for (int i = 0; i < j; i++) G[6 * i + j] = 0.0;
    for (int i = j + 1; i < 6; i++) {
      double s = A[6 * i + j];
      for (int k = 0; k < j; k++) s = s - G[6 * i + k] * G[6 * j + k];
      G[6 * i + j] = s / d;
    }
  }
}
__device__ static inline void fsub6(const double* G, double* v) {     // v <- G^-1 v
  for (int i = 0; i < 6; i++) {
    double s = v[i];
    for (int k = 0; k < i; k++) s = s - G[6 * i + k] * v[k];
    v[i] = s / G[7 * i];
  }
}
__device__ static inline void bsub6(const double* G, double* v) {     // v <- G^-T v
  for (int i = 5; i >= 0; i--) {
    double s = v[i];
    for (int k = i + 1; k < 6; k++) s = s - G[6 * k + i] * v[k];
    v[i] = s / G[7 * i];
  }
}
__device__ static inline void right_solve6(const double* Sb, const double* G, double* X) {   // X = Sb G^-T, row by row
  for (int r = 0; r < 6; r++) {
    double v[6];
    for (int c = 0; c < 6; c++) v[c] = Sb[6 * r + c];
    fsub6(G, v);
    for (int c = 0; c < 6; c++) X[6 * r + c] = v[c];
  }
}

// Block Thomas on the runs: lane (run, col) solves T y = column col of [b | C_left | C_right]; every lane of a run repeats the
// 6 x 6 factorisation, lane col 0 keeps the factors G (of the reduced diagonal block) and W = E G_prev^-T for the way back.
__global__ __launch_bounds__(64) void pgo_runs_kernel(int nruns, int nfree, const int* __restrict__ run_first,
                                                       const int* __restrict__ run_len, const int* __restrict__ sub,
                                                       const double* __restrict__ D, const double* __restrict__ bv,
                                                       const double* __restrict__ Eoff, double lambda, int only_b,
                                                       double* __restrict__ Gs, double* __restrict__ Ws, double* __restrict__ Y) {
  const int run = blockIdx.x * (64 / kPgoRunLanes) + threadIdx.x / kPgoRunLanes, col = threadIdx.x % kPgoRunLanes;
  const bool live = run < nruns && col < (only_b ? 1 : kPgoCols);   // only_b: the refinement pass, a new b against the same matrix
  const int f = live ? run_first[run] : 0, len = live ? run_len[run] : 0, l = f + len - 1;
  const int sleft = (live && f > 0) ? sub[f] : -1, sright = (live && l + 1 < nfree) ? sub[l + 1] : -1;
  double G[36], W[36], u[6];
  for (int k = 0; k < len; k++) {
    const int h = f + k;
    double Dk[36], z[6];
    for (int i = 0; i < 36; i++) Dk[i] = D[36 * (size_t)h + i];
    for (int i = 0; i < 6; i++) Dk[7 * i] = Dk[7 * i] + lambda;
    if (col == 0) for (int i = 0; i < 6; i++) z[i] = bv[6 * (size_t)h + i];
    else for (int i = 0; i < 6; i++) z[i] = 0.0;
    if (col >= 1 && col <= 6 && k == 0 && sleft >= 0)            // column col - 1 of the block (f, f - 1)
      for (int i = 0; i < 6; i++) z[i] = Eoff[36 * (size_t)sleft + 6 * i + (col - 1)];
    if (col >= 7 && k == len - 1 && sright >= 0)                 // column col - 7 of the block (l, l + 1) = row of the block (l + 1, l)
      for (int i = 0; i < 6; i++) z[i] = Eoff[36 * (size_t)sright + 6 * (col - 7) + i];
    if (k > 0) {
      const int s = sub[h];
      double Ek[36];
      for (int i = 0; i < 36; i++) Ek[i] = s >= 0 ? Eoff[36 * (size_t)s + i] : 0.0;
      right_solve6(Ek, G, W);
      for (int i = 0; i < 6; i++)
        for (int j = 0; j <= i; j++) {
          double acc = Dk[6 * i + j];
          for (int c = 0; c < 6; c++) acc = acc - W[6 * i + c] * W[6 * j + c];
          Dk[6 * i + j] = acc;
        }
      for (int i = 0; i < 6; i++) {
        double acc = z[i];
        for (int c = 0; c < 6; c++) acc = acc - W[6 * i + c] * u[c];
        z[i] = acc;
      }
      if (col == 0) for (int i = 0; i < 36; i++) Ws[36 * (size_t)h + i] = W[i];
    }
    chol6(Dk, G);
    if (col == 0) for (int i = 0; i < 36; i++) Gs[36 * (size_t)h + i] = G[i];
    fsub6(G, z);
    for (int i = 0; i < 6; i++) { u[i] = z[i]; Y[((size_t)h * kPgoCols + col) * 6 + i] = z[i]; }
  }
  __syncthreads();   // lane 0's factors are visible to the other lanes of its run
  double xn[6];
  for (int k = len - 1; k >= 0; k--) {
    const int h = f + k;
    double v[6];
    for (int i = 0; i < 6; i++) v[i] = Y[((size_t)h * kPgoCols + col) * 6 + i];
    if (k < len - 1)
      for (int i = 0; i < 6; i++) {
        double acc = v[i];
        for (int c = 0; c < 6; c++) acc = acc - Ws[36 * (size_t)(h + 1) + 6 * c + i] * xn[c];
        v[i] = acc;
      }
    for (int i = 0; i < 36; i++) G[i] = Gs[36 * (size_t)h + i];
    bsub6(G, v);
    for (int i = 0; i < 6; i++) { xn[i] = v[i]; Y[((size_t)h * kPgoCols + col) * 6 + i] = v[i]; }
  }
}

__host__ __device__ static inline size_t blk(int p, int q) { return ((size_t)p * (p + 1) / 2 + q) * 36; }

// Direct couplings between two junctions into the (zeroed) Schur matrix: one lane per such slot.
__global__ __launch_bounds__(64) void pgo_schur_scatter_kernel(int njj, const int* __restrict__ jj, const double* __restrict__ Eoff,
                                                                double* __restrict__ S) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= njj) return;
  const int s = jj[3 * t], p = jj[3 * t + 1], q = jj[3 * t + 2];
  for (int i = 0; i < 36; i++) S[blk(p, q) + i] = Eoff[36 * (size_t)s + i];
}

// One lane per junction q (Hessian index h): its diagonal block, its right-hand side and the block towards junction q - 1, each
// less what the neighbouring runs contribute: C^T T^-1 [b | C].
__global__ __launch_bounds__(64) void pgo_schur_kernel(int nj, int nfree, const int* __restrict__ jidx, const int* __restrict__ jpos,
                                                        const int* __restrict__ sub, const double* __restrict__ D,
                                                        const double* __restrict__ bv, const double* __restrict__ Eoff,
                                                        const double* __restrict__ Y, double lambda, int rhs_only,
                                                        double* __restrict__ S, double* __restrict__ rhs) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= nj) return;
  const int h = jidx[q];
  double Sq[36], r[6];
  for (int i = 0; i < 36; i++) Sq[i] = D[36 * (size_t)h + i];
  for (int i = 0; i < 6; i++) { Sq[7 * i] = Sq[7 * i] + lambda; r[i] = bv[6 * (size_t)h + i]; }
  if (h > 0 && jpos[h - 1] < 0 && sub[h] >= 0) {           // the run that ends at h - 1; ER = block (h, h - 1)
    const double* ER = Eoff + 36 * (size_t)sub[h];
    const double* Yl = Y + (size_t)(h - 1) * kPgoCols * 6;
    for (int i = 0; i < 6; i++) {
      for (int j = 0; j < 6; j++) {
        double acc = Sq[6 * i + j];
        for (int c = 0; c < 6; c++) acc = acc - ER[6 * i + c] * Yl[(7 + j) * 6 + c];
        Sq[6 * i + j] = acc;
      }
      double acc = r[i];
      for (int c = 0; c < 6; c++) acc = acc - ER[6 * i + c] * Yl[c];
      r[i] = acc;
    }
    if (q > 0 && !rhs_only) {   // towards the junction on the run's other side; a run that starts at index 0 has none and its columns are 0
      double* Sl = S + blk(q, q - 1);
      for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
          double acc = Sl[6 * i + j];
          for (int c = 0; c < 6; c++) acc = acc - ER[6 * i + c] * Yl[(1 + j) * 6 + c];
          Sl[6 * i + j] = acc;
        }
    }
  }
  if (h + 1 < nfree && jpos[h + 1] < 0 && sub[h + 1] >= 0) {   // the run that starts at h + 1; CL = block (h + 1, h)
    const double* CL = Eoff + 36 * (size_t)sub[h + 1];
    const double* Yf = Y + (size_t)(h + 1) * kPgoCols * 6;
    for (int i = 0; i < 6; i++) {
      for (int j = 0; j < 6; j++) {
        double acc = Sq[6 * i + j];
        for (int c = 0; c < 6; c++) acc = acc - CL[6 * c + i] * Yf[(1 + j) * 6 + c];
        Sq[6 * i + j] = acc;
      }
      double acc = r[i];
      for (int c = 0; c < 6; c++) acc = acc - CL[6 * c + i] * Yf[c];
      r[i] = acc;
    }
  }
  if (!rhs_only)
    for (int i = 0; i < 36; i++) S[blk(q, q) + i] = Sq[i];
  for (int i = 0; i < 6; i++) rhs[6 * (size_t)q + i] = r[i];
}

// Block column k of the dense Cholesky: lane (i, j), k <= j <= i < nj. It refactors the 6 x 6 pivot itself; j == k writes
// L(i, k), every other lane subtracts L(i, k) L(j, k)^T from S(i, j). Column k of S is only read here, columns > k only written.
__global__ __launch_bounds__(64) void pgo_chol_step_kernel(int nj, int k, double* __restrict__ S, double* __restrict__ L) {
  const int m = nj - k;
  const long long total = (long long)m * (m + 1) / 2;
  const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
  if (t >= total) return;
  int ii = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((long long)ii * (ii + 1) / 2 > t) ii--;
  while ((long long)(ii + 1) * (ii + 2) / 2 <= t) ii++;
  const int jj = (int)(t - (long long)ii * (ii + 1) / 2);
  const int i = k + ii, j = k + jj;
  double G[36], Li[36];
  chol6(S + blk(k, k), G);
  if (i == k) {
    for (int a = 0; a < 36; a++) L[blk(k, k) + a] = G[a];
    return;
  }
  right_solve6(S + blk(i, k), G, Li);
  if (j == k) {
    for (int a = 0; a < 36; a++) L[blk(i, k) + a] = Li[a];
    return;
  }
  double Lj[36];
  right_solve6(S + blk(j, k), G, Lj);
  double* Sij = S + blk(i, j);
  for (int a = 0; a < 6; a++)
    for (int b = 0; b < 6; b++) {
      double acc = Sij[6 * a + b];
      for (int c = 0; c < 6; c++) acc = acc - Li[6 * a + c] * Lj[6 * b + c];
      Sij[6 * a + b] = acc;
    }
}

// L L^T x = rhs on one workgroup: column-oriented forward substitution, row-oriented backward; x replaces rhs.
__global__ __launch_bounds__(256) void pgo_trisolve_kernel(int nj, const double* __restrict__ L, double* __restrict__ x) {
  for (int k = 0; k < nj; k++) {
    if (threadIdx.x == 0) fsub6(L + blk(k, k), x + 6 * (size_t)k);
    __syncthreads();
    for (int i = k + 1 + threadIdx.x; i < nj; i += 256) {
      const double* Lik = L + blk(i, k);
      for (int a = 0; a < 6; a++) {
        double acc = x[6 * (size_t)i + a];
        for (int c = 0; c < 6; c++) acc = acc - Lik[6 * a + c] * x[6 * (size_t)k + c];
        x[6 * (size_t)i + a] = acc;
      }
    }
    __syncthreads();
  }
  for (int k = nj - 1; k >= 0; k--) {
    if (threadIdx.x == 0) bsub6(L + blk(k, k), x + 6 * (size_t)k);
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += 256) {
      const double* Lkj = L + blk(k, j);
      for (int a = 0; a < 6; a++) {
        double acc = x[6 * (size_t)j + a];
        for (int c = 0; c < 6; c++) acc = acc - Lkj[6 * c + a] * x[6 * (size_t)k + c];
        x[6 * (size_t)j + a] = acc;
      }
    }
    __syncthreads();
  }
}

// The residual b - (A + lambda I) x of one free vertex's rows, A's lower triangle mirrored, accumulated in twice the working
// precision (two_prod by fma, two_sum) and rounded once: the right-hand side of the refinement pass. adj lists the vertex's
// off-diagonal blocks: slot * 2 + (1 when the vertex is the block's column, so the block acts transposed).
__global__ __launch_bounds__(64) void pgo_residual_kernel(int nfree, const int* __restrict__ adj_ptr, const int* __restrict__ adj,
                                                           const int* __restrict__ slot_rc, const double* __restrict__ D,
                                                           const double* __restrict__ Eoff, const double* __restrict__ bv,
                                                           const double* __restrict__ x, double lambda, double* __restrict__ rv) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= nfree) return;
  double hi[6], lo[6];
  for (int i = 0; i < 6; i++) { hi[i] = bv[6 * (size_t)h + i]; lo[i] = 0.0; }
  auto sub_prod = [&](int i, double a, double b) {   // (hi, lo)[i] -= a * b
    const double p = -(a * b), pe = -fma(a, b, -(a * b));
    const double sum = hi[i] + p, bb = sum - hi[i];
    const double err = (hi[i] - (sum - bb)) + (p - bb);
    hi[i] = sum;
    lo[i] = lo[i] + (err + pe);
  };
  const double* Dh = D + 36 * (size_t)h;
  const double* xh = x + 6 * (size_t)h;
  for (int i = 0; i < 6; i++) {
    for (int j = 0; j < 6; j++) sub_prod(i, i >= j ? Dh[6 * i + j] : Dh[6 * j + i], xh[j]);
    sub_prod(i, lambda, xh[i]);
  }
  for (int p = adj_ptr[h]; p < adj_ptr[h + 1]; p++) {
    const int code = adj[p], sl = code >> 1;
    const double* E = Eoff + 36 * (size_t)sl;
    const double* xo = x + 6 * (size_t)((code & 1) ? slot_rc[2 * sl] : slot_rc[2 * sl + 1]);
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) sub_prod(i, (code & 1) ? E[6 * j + i] : E[6 * i + j], xo[j]);
  }
  for (int i = 0; i < 6; i++) rv[6 * (size_t)h + i] = hi[i] + lo[i];
}

// x of every free vertex (a junction's comes from the Schur solve, a run vertex's from its three column groups). First pass
// (refine 0): x is stored, nothing else. Refinement pass (refine 1): what was solved is the correction; x += it, then oplus on
// the pose and the vertex's term of scaleLambda's sum.
__global__ __launch_bounds__(64) void pgo_update_kernel(int nfree, const int* __restrict__ jpos, const int* __restrict__ vrun,
                                                         const int* __restrict__ run_first, const int* __restrict__ run_len,
                                                         const int* __restrict__ vfree, const double* __restrict__ Y,
                                                         const double* __restrict__ xj, const double* __restrict__ bv, double lambda,
                                                         int refine, double* __restrict__ x, double* __restrict__ poses,
                                                         double* __restrict__ dotp) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= nfree) return;
  double v[6];
  if (jpos[h] >= 0) {
    for (int i = 0; i < 6; i++) v[i] = xj[6 * (size_t)jpos[h] + i];
  } else {
    const int run = vrun[h], f = run_first[run], l = f + run_len[run] - 1;
    const double* Yh = Y + (size_t)h * kPgoCols * 6;
    for (int i = 0; i < 6; i++) v[i] = Yh[i];
    if (f > 0) {
      const double* xl = xj + 6 * (size_t)jpos[f - 1];
      for (int i = 0; i < 6; i++)
        for (int c = 0; c < 6; c++) v[i] = v[i] - Yh[(1 + c) * 6 + i] * xl[c];
    }
    if (l + 1 < nfree) {
      const double* xr = xj + 6 * (size_t)jpos[l + 1];
      for (int i = 0; i < 6; i++)
        for (int c = 0; c < 6; c++) v[i] = v[i] - Yh[(7 + c) * 6 + i] * xr[c];
    }
  }
  if (!refine) {
    for (int i = 0; i < 6; i++) x[6 * (size_t)h + i] = v[i];
    return;
  }
  for (int i = 0; i < 6; i++) v[i] = x[6 * (size_t)h + i] + v[i];
  double dsum = 0.0;
  for (int i = 0; i < 6; i++) {
    x[6 * (size_t)h + i] = v[i];
    dsum = dsum + v[i] * (lambda * v[i] + bv[6 * (size_t)h + i]);
  }
  dotp[h] = dsum;
  // Vertex::oplus: fromCompactQuaternion returns the identity when 1 - |v|^2 < 0; the translation still applies
  Rt inc;
  double w = 1 - ((v[3] * v[3] + v[4] * v[4]) + v[5] * v[5]);
  if (w < 0) {
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) inc.R[i][j] = i == j ? 1.0 : 0.0;
  } else {
    w = sqrt(w);
    const double qx = v[3], qy = v[4], qz = v[5];
    const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy,
                 tzz = tz * qz;
    inc.R[0][0] = 1 - (tyy + tzz); inc.R[0][1] = txy - twz; inc.R[0][2] = txz + twy;
    inc.R[1][0] = txy + twz; inc.R[1][1] = 1 - (txx + tzz); inc.R[1][2] = tyz - twx;
    inc.R[2][0] = txz - twy; inc.R[2][1] = tyz + twx; inc.R[2][2] = 1 - (txx + tyy);
  }
  for (int i = 0; i < 3; i++) inc.t[i] = v[i];
  double* P = poses + 12 * (size_t)vfree[h];
  store_rt(compose(load_rt(P), inc), P);
}

// ---- one optimisation on the device ------------------------------------------------------------------------------------------------
struct PgoDev {   // where the pieces of one call lie in the handle's buffers
  int *vi, *vj, *hidx, *inc_ptr, *inc, *slot_ptr, *slot_edge, *sub, *jpos, *jidx, *vrun, *run_first, *run_len, *jj, *vfree, *adj_ptr, *adj, *slot_rc, *order;
  double *poses, *meas, *info, *rec, *chi, *scal, *D, *bv, *Eoff, *Gs, *Ws, *Y, *x, *dotp, *S, *L, *xj, *rv;
};

// Where one optimisation reads its arrays and leaves its poses. Host memory: poses in ascending id order. The caller's device
// memory: poses in the caller's vertex order (the gather kernel sorts them). Measurements and information in edge order; the
// optimised poses go to poses_out in ascending id order.
struct PgoIO { const double *poses, *meas, *info; double* poses_out; bool device; };

__global__ __launch_bounds__(64) void pgo_gather_poses_kernel(int nv, const int* __restrict__ order, const double* __restrict__ src,
                                                               double* __restrict__ dst) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= nv * 12) return;
  dst[t] = src[12 * (size_t)order[t / 12] + t % 12];
}

// num iterations of HyperGraph::optimize on the poses of io, then computeActiveErrors. edge_chi (host memory, may be null)
// receives the final per-edge chi2. Edges arrive as the plan's vi / vj with meas / info in edge order.
static int pgo_optimize(sbm_handle* h, const PgoPlan& P, int num, const PgoIO& io, double* err, double* edge_chi) {
  StageClock& clk = h->pgo.clock;
  hipStream_t s = h->stream;
  HIPCHK(h, clk.start(pgo_stages(), h->profiling != 0));
  const int nv = P.nv, ne = P.ne, nf = P.nfree, nj = P.nj;
  const size_t nS = blk(nj, 0);
  // before any buffer is replaced: a call that fails below leaves nothing for sbm_pgo_debug_fetch to copy from
  h->pgo.last = PgoLast{ne, nf, P.nslots, nj, P.nruns, 0, 0.0, PgoDebug{}};
  PgoDev d;
  HIPCHK(h, carve(h->pgo.graph, s, [&](Carve& c) {
    P.each_index(d, [&](const std::vector<int>& v, int*& p) { p = c.take<int>(v.size()); });
    d.poses = c.take<double>(12 * (size_t)nv);
    d.meas = c.take<double>(12 * (size_t)ne);
    d.info = c.take<double>(36 * (size_t)ne);
  }));
  HIPCHK(h, carve(h->pgo.edge, s, [&](Carve& c) {
    d.scal = c.take<double>(8);          // chi2, scaleLambda's sum, max_diag
    d.chi = c.take<double>(std::max(ne, 1));
    d.rec = c.take<double>((size_t)kRec * std::max(ne, 1));
  }));
  HIPCHK(h, carve(h->pgo.sys, s, [&](Carve& c) {
    d.D = c.take<double>(36 * (size_t)nf);
    d.Gs = c.take<double>(36 * (size_t)nf);
    d.Ws = c.take<double>(36 * (size_t)nf);
    d.Eoff = c.take<double>(36 * (size_t)std::max(P.nslots, 1));
    d.bv = c.take<double>(6 * (size_t)nf);
    d.Y = c.take<double>((size_t)nf * kPgoCols * 6);
    d.x = c.take<double>(6 * (size_t)nf);
    d.dotp = c.take<double>(nf);
    d.xj = c.take<double>(6 * (size_t)nj);
    d.rv = c.take<double>(6 * (size_t)nf);
  }));
  HIPCHK(h, carve(h->pgo.schur, s, [&](Carve& c) {
    d.S = c.take<double>(std::max(nS, (size_t)36));
    d.L = c.take<double>(std::max(nS, (size_t)36));
  }));
  hipError_t up = hipSuccess;
  P.each_index(d, [&](const std::vector<int>& v, int* p) {
    if (up == hipSuccess && !v.empty()) up = hipMemcpyAsync(p, v.data(), 4 * v.size(), hipMemcpyHostToDevice, s);
  });
  HIPCHK(h, up);
  const hipMemcpyKind in = io.device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                      out = io.device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (io.device) {
    hipLaunchKernelGGL(pgo_gather_poses_kernel, dim3((nv * 12 + 63) / 64), dim3(64), 0, s, nv, d.order, io.poses, d.poses);
    HIPCHK(h, hipGetLastError());
  } else {
    HIPCHK(h, hipMemcpyAsync(d.poses, io.poses, 96 * (size_t)nv, in, s));
  }
  if (ne) {
    HIPCHK(h, hipMemcpyAsync(d.meas, io.meas, 96 * (size_t)ne, in, s));
    HIPCHK(h, hipMemcpyAsync(d.info, io.info, 288 * (size_t)ne, in, s));
  }
  HIPCHK(h, hipMemsetAsync(d.scal, 0, 64, s));
  double scal[3] = {0, 0, 0}, lambda = 0.0, chi_prev = 0.0, dot_prev = 0.0;
  const dim3 b64(64);
  for (int it = 0; it < num && nf > 0; it++) {
    const bool last = it == num - 1;
    if (last) HIPCHK(h, clk.mark(kPgBegin, s));
    if (ne) {
      hipLaunchKernelGGL(pgo_linearise_kernel, dim3((ne + 63) / 64), b64, 0, s, ne, d.vi, d.vj, d.hidx, d.poses, d.meas, d.info, 0,
                         d.rec, d.chi, d.scal);
      HIPCHK(h, hipGetLastError());
    }
    hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, s, d.chi, ne, d.scal);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(scal, d.scal, sizeof(scal), hipMemcpyDeviceToHost, s));   // chi2 and the last step's sum come home
    HIPCHK(h, hipStreamSynchronize(s));
    if (it == 0) {
      lambda = 1e-5 * scal[2];   // tau * max_diag, max_diag as the LAST edge's constructQuadraticForm leaves it
    } else {                     // scaleLambda, as written; there is no step rejection
      const double rho = (chi_prev - scal[0]) / (dot_prev + 1e-3);
      double alpha = 1. - pow((2 * rho - 1), 3);
      alpha = (std::min)(alpha, 2. / 3.);
      lambda *= (std::max)(1. / 3., alpha);
    }
    chi_prev = scal[0];
    if (last) HIPCHK(h, clk.mark(kPgLinearised, s));
    hipLaunchKernelGGL(pgo_assemble_kernel, dim3((nf + P.nslots + 63) / 64), b64, 0, s, nf, P.nslots, d.inc_ptr, d.inc, d.slot_ptr,
                       d.slot_edge, d.rec, d.D, d.bv, d.Eoff);
    HIPCHK(h, hipGetLastError());
    if (last) HIPCHK(h, clk.mark(kPgAssembled, s));
    // the solve, then one step of iterative refinement: the residual in twice the working precision against the same factors
    for (int pass = 0; pass < 2; pass++) {
      const double* rhs = pass ? d.rv : d.bv;
      if (P.nruns) {
        hipLaunchKernelGGL(pgo_runs_kernel, dim3((P.nruns + 3) / 4), b64, 0, s, P.nruns, nf, d.run_first, d.run_len, d.sub, d.D, rhs,
                           d.Eoff, lambda, pass, d.Gs, d.Ws, d.Y);
        HIPCHK(h, hipGetLastError());
      }
      if (nj) {
        if (!pass) {
          HIPCHK(h, hipMemsetAsync(d.S, 0, 8 * nS, s));
          if (!P.jj.empty()) {
            const int njj = (int)P.jj.size() / 3;
            hipLaunchKernelGGL(pgo_schur_scatter_kernel, dim3((njj + 63) / 64), b64, 0, s, njj, d.jj, d.Eoff, d.S);
            HIPCHK(h, hipGetLastError());
          }
        }
        hipLaunchKernelGGL(pgo_schur_kernel, dim3((nj + 63) / 64), b64, 0, s, nj, nf, d.jidx, d.jpos, d.sub, d.D, rhs, d.Eoff, d.Y,
                           lambda, pass, d.S, d.xj);
        HIPCHK(h, hipGetLastError());
        for (int k = 0; k < nj && !pass; k++) {
          const long long m = nj - k, total = m * (m + 1) / 2;
          hipLaunchKernelGGL(pgo_chol_step_kernel, dim3((unsigned)((total + 63) / 64)), b64, 0, s, nj, k, d.S, d.L);
        }
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL(pgo_trisolve_kernel, dim3(1), dim3(256), 0, s, nj, d.L, d.xj);
        HIPCHK(h, hipGetLastError());
      }
      if (pass && last) HIPCHK(h, clk.mark(kPgSolved, s));
      hipLaunchKernelGGL(pgo_update_kernel, dim3((nf + 63) / 64), b64, 0, s, nf, d.jpos, d.vrun, d.run_first, d.run_len, d.vfree, d.Y,
                         d.xj, d.bv, lambda, pass, d.x, d.poses, d.dotp);
      HIPCHK(h, hipGetLastError());
      if (!pass) {
        hipLaunchKernelGGL(pgo_residual_kernel, dim3((nf + 63) / 64), b64, 0, s, nf, d.adj_ptr, d.adj, d.slot_rc, d.D, d.Eoff, d.bv,
                           d.x, lambda, d.rv);
        HIPCHK(h, hipGetLastError());
      }
    }
    hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, s, d.dotp, nf, d.scal + 1);
    HIPCHK(h, hipGetLastError());
    if (last) HIPCHK(h, clk.mark(kPgEnd, s));
    HIPCHK(h, hipMemcpyAsync(&dot_prev, d.scal + 1, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    h->pgo.last.iterations = it + 1;
    h->pgo.last.lambda = lambda;
    if (last) {
      HIPCHK(h, clk.add(kPgLinearise, kPgBegin, kPgLinearised));
      HIPCHK(h, clk.add(kPgAssemble, kPgLinearised, kPgAssembled));
      HIPCHK(h, clk.add(kPgSolve, kPgAssembled, kPgSolved));
      HIPCHK(h, clk.add(kPgUpdate, kPgSolved, kPgEnd));
      if (clk.on) clk.ms[kPgTotal] = ((clk.ms[kPgLinearise] + clk.ms[kPgAssemble]) + clk.ms[kPgSolve]) + clk.ms[kPgUpdate];
    }
  }
  // computeActiveErrors at the final poses; the records of the last linearisation stay for sbm_pgo_debug_fetch
  if (ne) {
    hipLaunchKernelGGL(pgo_linearise_kernel, dim3((ne + 63) / 64), b64, 0, s, ne, d.vi, d.vj, d.hidx, d.poses, d.meas, d.info, 1,
                       d.rec, d.chi, d.scal);
    HIPCHK(h, hipGetLastError());
  }
  hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, s, d.chi, ne, d.scal);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(scal, d.scal, sizeof(scal), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(io.poses_out, d.poses, 96 * (size_t)nv, out, s));
  if (edge_chi && ne) HIPCHK(h, hipMemcpyAsync(edge_chi, d.chi, 8 * (size_t)ne, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  *err = scal[0];
  h->pgo.last.dev = PgoDebug{d.rec, d.D, d.Eoff, d.bv, d.x};
  return SBM_OK;
}

}  // namespace sbm

using namespace sbm;

// runOptimize on the graph's arrays, host memory or (device) the caller's device memory: check, plan, optimise, and the plan for
// sbm_pgo_last_plan. The host form's poses go up in ascending id order.
static int pgo_run(sbm_handle* h, const sbm_pgo_params* p, const sbm_pgo_graph* g, bool device, double* poses_out, double* err) {
  if (!h || !poses_out || !err) return SBM_ERR_NULL;
  int st = pgo_check(p, g, !device);
  if (st != SBM_OK) return st;
  try {
    PgoPlan P;
    st = pgo_make_plan(p, g, P);
    if (st != SBM_OK) return st;
    std::vector<double> sorted(device ? 0 : 12 * (size_t)P.nv);
    for (int i = 0; !device && i < P.nv; i++) memcpy(&sorted[12 * (size_t)i], g->poses + 12 * (size_t)P.order[i], 96);
    DeviceScope dscope(h->device);
    HIPCHK(h, dscope.enter());
    st = pgo_optimize(h, P, p->num, PgoIO{device ? g->poses : sorted.data(), g->meas, g->info, poses_out, device}, err, nullptr);
    if (st != SBM_OK) return st;
    pgo_plan_info(P, &h->pgo.plan);
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  return SBM_OK;
}

extern "C" {

int sbm_pgo_optimize(sbm_handle* h, const sbm_pgo_params* p, const sbm_pgo_graph* g, double* poses_out, double* err) {
  return pgo_run(h, p, g, false, poses_out, err);
}

int sbm_pgo_optimize_device(sbm_handle* h, const sbm_pgo_params* p, const sbm_pgo_graph* g, void* d_poses_out, double* err) {
  return pgo_run(h, p, g, true, (double*)d_poses_out, err);
}

// The robust loop propagates poses on the host, so poses and measurements come home once; every iteration is the host form's.
int sbm_pgo_optimize_robust_device(sbm_handle* h, const sbm_pgo_params* p, const sbm_pgo_graph* g, int32_t* n_out, int32_t* ids_out,
                                   void* d_poses_out, double* err, int32_t* removed, int32_t removed_cap, int32_t* n_removed) {
  if (!h || !d_poses_out || !n_out) return SBM_ERR_NULL;
  int st = pgo_check(p, g, false);
  if (st != SBM_OK) return st;
  try {
    std::vector<double> poses(12 * (size_t)g->n_vertices), meas(12 * (size_t)g->n_edges + 1), info(36 * (size_t)g->n_edges + 1),
        out(12 * (size_t)g->n_vertices);
    {
      DeviceScope dscope(h->device);
      HIPCHK(h, dscope.enter());
      HIPCHK(h, hipStreamSynchronize(h->stream));
      HIPCHK(h, hipMemcpy(poses.data(), g->poses, 8 * poses.size(), hipMemcpyDeviceToHost));
      if (g->n_edges) {
        HIPCHK(h, hipMemcpy(meas.data(), g->meas, 96 * (size_t)g->n_edges, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(info.data(), g->info, 288 * (size_t)g->n_edges, hipMemcpyDeviceToHost));
      }
    }
    sbm_pgo_graph hg = *g;
    hg.poses = poses.data(); hg.meas = meas.data(); hg.info = info.data();
    st = sbm_pgo_optimize_robust(h, p, &hg, n_out, ids_out, out.data(), err, removed, removed_cap, n_removed);
    if (st != SBM_OK) return st;
    DeviceScope dscope(h->device);
    HIPCHK(h, dscope.enter());
    HIPCHK(h, hipMemcpy(d_poses_out, out.data(), 96 * (size_t)*n_out, hipMemcpyHostToDevice));
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  return SBM_OK;
}

int sbm_pgo_optimize_robust(sbm_handle* h, const sbm_pgo_params* p, const sbm_pgo_graph* g, int32_t* n_out, int32_t* ids_out,
                            double* poses_out, double* err, int32_t* removed, int32_t removed_cap, int32_t* n_removed) {
  if (!h || !n_out || !ids_out || !poses_out || !err || !n_removed || (removed_cap > 0 && !removed)) return SBM_ERR_NULL;
  int st = pgo_check(p, g);
  if (st != SBM_OK) return st;
  if (removed_cap < 0) return SBM_ERR_SIZE;
  try {
    std::map<int, Rt> in, out;
    for (int i = 0; i < g->n_vertices; i++) in[g->ids[i]] = load_rt(g->poses + 12 * (size_t)i);
    PgoLinks alive;
    alive.from.assign(g->from, g->from + g->n_edges);
    alive.to.assign(g->to, g->to + g->n_edges);
    alive.meas.assign(g->meas, g->meas + 12 * (size_t)g->n_edges);
    alive.info.assign(g->info, g->info + 36 * (size_t)g->n_edges);
    DeviceScope dscope(h->device);
    HIPCHK(h, dscope.enter());
    *n_removed = 0;
    while (true) {
      std::vector<int> kept;
      pgo_connected(p->fixed_id, in, alive, out, kept);
      PgoLinks sel;
      for (int k : kept) sel.append(alive, (size_t)k);
      std::vector<int> ids;
      std::vector<double> poses0;
      for (const auto& kv : out) {
        ids.push_back(kv.first);
        poses0.resize(poses0.size() + 12);
        store_rt(kv.second, &poses0[poses0.size() - 12]);
      }
      sbm_pgo_graph sg = {(int32_t)ids.size(), ids.data(), poses0.data(), (int32_t)sel.from.size(), sel.from.data(), sel.to.data(),
                          sel.meas.data(), sel.info.data()};
      PgoPlan P;
      st = pgo_make_plan(p, &sg, P);
      if (st != SBM_OK) return st;
      std::vector<double> poses5(poses0.size()), chi(sel.size() + 1);
      double e5;
      st = pgo_optimize(h, P, 5, PgoIO{poses0.data(), sel.meas.data(), sel.info.data(), poses5.data(), false}, &e5, chi.data());
      if (st != SBM_OK) return st;
      int worst = -1;
      double werr = 0;
      for (size_t k = 0; k < sel.from.size(); k++) {
        const int a = sel.from[k], b = sel.to[k];
        if (a != b + 1 && b != a + 1 && chi[k] >= 10.0 && chi[k] > werr) { worst = (int)k; werr = chi[k]; }
      }
      if (worst < 0) {   // runOptimize from the re-propagated poses, not from the five-iteration result
        st = pgo_optimize(h, P, p->num, PgoIO{poses0.data(), sel.meas.data(), sel.info.data(), poses_out, false}, err, nullptr);
        if (st != SBM_OK) return st;
        pgo_plan_info(P, &h->pgo.plan);
        *n_out = (int32_t)ids.size();
        memcpy(ids_out, ids.data(), 4 * ids.size());
        return SBM_OK;
      }
      const int a = sel.from[(size_t)worst], b = sel.to[(size_t)worst];
      if (*n_removed < removed_cap) { removed[2 * *n_removed] = a; removed[2 * *n_removed + 1] = b; }
      ++*n_removed;
      PgoLinks next;
      for (size_t k = 0; k < sel.size(); k++)
        if (sel.from[k] != a || sel.to[k] != b) next.append(sel, k);   // every link with that (from, to) goes
      alive = std::move(next);
    }
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
}

int sbm_pgo_last_plan(sbm_handle* h, sbm_pgo_plan_info* info, double* lambda, int32_t* iterations) {
  if (!h || !info) return SBM_ERR_NULL;
  *info = h->pgo.plan;
  if (lambda) *lambda = h->pgo.last.lambda;
  if (iterations) *iterations = h->pgo.last.iterations;
  return SBM_OK;
}

int sbm_pgo_debug_fetch(sbm_handle* h, int which, void* dst, size_t dst_bytes) {
  if (!h || !dst) return SBM_ERR_NULL;
  const auto& L = h->pgo.last;
  if (!L.dev.rec) return SBM_ERR_UNSUPPORTED;
  const void* src = nullptr;
  size_t n = 0;
  switch (which) {
    case SBM_PGO_DEBUG_EDGES: src = L.dev.rec; n = 8 * (size_t)kRec * L.ne; break;
    case SBM_PGO_DEBUG_DIAG: src = L.dev.D; n = 288 * (size_t)L.nfree; break;
    case SBM_PGO_DEBUG_OFFDIAG: src = L.dev.Eoff; n = 288 * (size_t)L.nslots; break;
    case SBM_PGO_DEBUG_B: src = L.dev.bv; n = 48 * (size_t)L.nfree; break;
    case SBM_PGO_DEBUG_X: src = L.dev.x; n = 48 * (size_t)L.nfree; break;
    default: return SBM_ERR_UNSUPPORTED;
  }
  if (dst_bytes < n) return SBM_ERR_SIZE;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (n) HIPCHK(h, hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
  return SBM_OK;
}

}  // extern "C"
