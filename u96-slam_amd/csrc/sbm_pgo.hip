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
// The partition into runs and junctions is host code (PgoPlan) and needs no device.
#include <math.h>

#include <cmath>
#include <algorithm>
#include <map>
#include <new>
#include <vector>

#include "sbm_handle.h"

#pragma clang fp contract(off)

namespace sbm {

constexpr int kPgoMaxJunctions = 1024;   // the dense Schur complement is (6 * 1024)^2 doubles at most, twice (S and its factor)
constexpr int kPgoRunLanes = 16;         // lanes per run: 13 right-hand columns, 3 idle
constexpr int kPgoCols = 13;             // b, the 6 columns towards the left junction, the 6 towards the right one

enum PgoStage { kPgLinearise, kPgAssemble, kPgSolve, kPgUpdate, kPgTotal, kPgStageCount };
enum PgoMark { kPgBegin, kPgLinearised, kPgAssembled, kPgSolved, kPgEnd, kPgMarkCount };
static const char* const kPgoNames[] = {"pgo_linearise", "pgo_assemble", "pgo_solve", "pgo_update", "pgo_total"};
StageTable pgo_stages() { return stage_table<kPgStageCount, kPgMarkCount>(kPgoNames); }

// ---- 3x3 / 6x6 arithmetic, every sum left to right ------------------------------------------------------------------------------
struct Rt { double R[3][3], t[3]; };

__host__ __device__ static inline double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}
__host__ __device__ static inline void mul33(const double A[3][3], const double B[3][3], double C[3][3]) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[i][j] = dot3(A[i][0], A[i][1], A[i][2], B[0][j], B[1][j], B[2][j]);
}
__host__ __device__ static inline void mul3v(const double A[3][3], const double v[3], double o[3]) {
  for (int i = 0; i < 3; i++) o[i] = dot3(A[i][0], A[i][1], A[i][2], v[0], v[1], v[2]);
}
__host__ __device__ static inline Rt load_rt(const double* p) {
  Rt r;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) r.R[i][j] = p[4 * i + j];
    r.t[i] = p[4 * i + 3];
  }
  return r;
}
__host__ __device__ static inline void store_rt(const Rt& r, double* p) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) p[4 * i + j] = r.R[i][j];
    p[4 * i + 3] = r.t[i];
  }
}
__host__ __device__ static inline Rt inverse(const Rt& a) {
  Rt r;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) r.R[i][j] = a.R[j][i];
  double v[3];
  mul3v(r.R, a.t, v);
  for (int i = 0; i < 3; i++) r.t[i] = -v[i];
  return r;
}
__host__ __device__ static inline Rt compose(const Rt& a, const Rt& b) {
  Rt r;
  mul33(a.R, b.R, r.R);
  double v[3];
  mul3v(a.R, b.t, v);
  for (int i = 0; i < 3; i++) r.t[i] = v[i] + a.t[i];
  return r;
}

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

// ---- the partition: host code, no device ------------------------------------------------------------------------------------------
struct PgoPlan {
  int nv = 0, ne = 0, nfree = 0, nslots = 0, nruns = 0, nj = 0, ncoupling = 0, longest = 0;
  std::vector<int> order;        // sorted position -> caller's vertex position
  std::vector<int> ids;          // ascending
  std::vector<int> hidx;         // per sorted vertex: Hessian index, -1 for the fixed one
  std::vector<int> vfree;        // Hessian index -> sorted vertex
  std::vector<int> vi, vj;       // per edge: sorted vertex of from / to
  std::vector<uint8_t> couples;  // per edge
  std::vector<int> inc_ptr, inc, slot_ptr, slot_edge, slot_rc;   // slot_rc: (row, col) Hessian indices, row > col
  std::vector<int> sub;          // per Hessian index h: the slot of (h, h - 1) or -1
  std::vector<int> jpos, jidx, vrun, run_first, run_len, jj;
  std::vector<int> adj_ptr, adj;  // per Hessian index: its off-diagonal blocks, slot * 2 + (1 when it is the block's column)
};

// host_arrays: poses, meas and info are host memory and are read; the device forms check ids and topology only
static int pgo_check(const sbm_pgo_params* p, const sbm_pgo_graph* g, bool host_arrays = true) {
  if (!p || !g) return SBM_ERR_NULL;
  if (p->num < 0) return SBM_ERR_SIZE;
  if (p->coupling != SBM_PGO_COUPLING_REFERENCE && p->coupling != SBM_PGO_COUPLING_SYMMETRIC) return SBM_ERR_UNSUPPORTED;
  if (p->run_max < 1 || p->run_max > 65536) return SBM_ERR_UNSUPPORTED;
  if (g->n_vertices <= 0 || g->n_edges < 0) return SBM_ERR_SIZE;              // an empty graph
  if (!g->ids || !g->poses || (g->n_edges > 0 && (!g->from || !g->to || !g->meas || !g->info))) return SBM_ERR_NULL;
  for (size_t i = 0; host_arrays && i < 12 * (size_t)g->n_vertices; i++)
    if (!std::isfinite(g->poses[i])) return SBM_ERR_UNSUPPORTED;
  for (size_t i = 0; host_arrays && i < 12 * (size_t)g->n_edges; i++)
    if (!std::isfinite(g->meas[i])) return SBM_ERR_UNSUPPORTED;
  for (size_t i = 0; host_arrays && i < 36 * (size_t)g->n_edges; i++)
    if (!std::isfinite(g->info[i])) return SBM_ERR_UNSUPPORTED;
  try {
    std::vector<int> ids(g->ids, g->ids + g->n_vertices);
    std::sort(ids.begin(), ids.end());
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return SBM_ERR_SIZE;   // a vertex id given twice
    if (!std::binary_search(ids.begin(), ids.end(), p->fixed_id)) return SBM_ERR_SIZE;  // an absent fixed_id
    for (int k = 0; k < g->n_edges; k++) {
      if (g->from[k] == g->to[k]) return SBM_ERR_UNSUPPORTED;
      if (!std::binary_search(ids.begin(), ids.end(), g->from[k]) || !std::binary_search(ids.begin(), ids.end(), g->to[k]))
        return SBM_ERR_SIZE;                                                            // an edge naming an absent vertex
    }
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  return SBM_OK;
}

// The partition of a checked graph. Junctions: both ends of every coupling between Hessian indices that are not neighbours, and
// every (run_max + 1)-th vertex of a longer stretch. Runs: the maximal stretches of consecutive indices between junctions.
static int pgo_make_plan(const sbm_pgo_params* p, const sbm_pgo_graph* g, PgoPlan& P) {
  try {
    const int nv = g->n_vertices, ne = g->n_edges;
    P.nv = nv; P.ne = ne;
    P.order.resize(nv);
    for (int i = 0; i < nv; i++) P.order[i] = i;
    std::sort(P.order.begin(), P.order.end(), [&](int a, int b) { return g->ids[a] < g->ids[b]; });
    P.ids.resize(nv); P.hidx.resize(nv);
    for (int i = 0; i < nv; i++) {
      P.ids[i] = g->ids[P.order[i]];
      P.hidx[i] = P.ids[i] == p->fixed_id ? -1 : P.nfree++;
      if (P.hidx[i] >= 0) P.vfree.push_back(i);
    }
    const int nf = P.nfree;
    P.vi.resize(ne); P.vj.resize(ne); P.couples.assign(ne, 0);
    std::vector<std::vector<int>> inc(nf);
    std::map<std::pair<int, int>, std::vector<int>> slots;
    for (int k = 0; k < ne; k++) {
      P.vi[k] = (int)(std::lower_bound(P.ids.begin(), P.ids.end(), g->from[k]) - P.ids.begin());
      P.vj[k] = (int)(std::lower_bound(P.ids.begin(), P.ids.end(), g->to[k]) - P.ids.begin());
      const int hi = P.hidx[P.vi[k]], hj = P.hidx[P.vj[k]];
      if (hi >= 0) inc[hi].push_back(2 * k);
      if (hj >= 0) inc[hj].push_back(2 * k + 1);
      // the one off-diagonal block, at (to, from): SimplicialLDLT reads it only from the lower triangle; where `to` is fixed
      // the reference forms a negative index, here the coupling is dropped
      const bool both = hi >= 0 && hj >= 0;
      if (both && (hj > hi || p->coupling == SBM_PGO_COUPLING_SYMMETRIC)) {
        P.couples[k] = 1;
        P.ncoupling++;
        if (hj > hi) slots[{hj, hi}].push_back(2 * k);        // m^T
        else slots[{hi, hj}].push_back(2 * k + 1);            // mirrored from the upper triangle: m
      }
    }
    P.inc_ptr.assign(nf + 1, 0);
    for (int h = 0; h < nf; h++) {
      P.inc_ptr[h + 1] = P.inc_ptr[h] + (int)inc[h].size();
      P.inc.insert(P.inc.end(), inc[h].begin(), inc[h].end());
    }
    P.sub.assign(nf, -1);
    P.jpos.assign(nf, -1);
    P.slot_ptr.push_back(0);
    for (const auto& s : slots) {
      const int r = s.first.first, c = s.first.second;
      if (r - c == 1) P.sub[r] = P.nslots;
      else P.jpos[r] = P.jpos[c] = 0;                          // marked; numbered below
      P.slot_rc.push_back(r); P.slot_rc.push_back(c);
      P.slot_edge.insert(P.slot_edge.end(), s.second.begin(), s.second.end());
      P.slot_ptr.push_back((int)P.slot_edge.size());
      P.nslots++;
    }
    int streak = 0;
    for (int h = 0; h < nf; h++) {
      if (P.jpos[h] >= 0) { streak = 0; continue; }
      if (++streak > p->run_max) { P.jpos[h] = 0; streak = 0; }
    }
    P.vrun.assign(nf, -1);
    for (int h = 0; h < nf; h++) {
      if (P.jpos[h] >= 0) { P.jpos[h] = P.nj++; P.jidx.push_back(h); continue; }
      if (h == 0 || P.jpos[h - 1] >= 0) { P.run_first.push_back(h); P.run_len.push_back(0); P.nruns++; }
      P.vrun[h] = P.nruns - 1;
      P.longest = std::max(P.longest, ++P.run_len.back());
    }
    std::vector<std::vector<int>> adj(nf);
    for (int s = 0; s < P.nslots; s++) {
      adj[P.slot_rc[2 * s]].push_back(2 * s);
      adj[P.slot_rc[2 * s + 1]].push_back(2 * s + 1);
    }
    P.adj_ptr.assign(nf + 1, 0);
    for (int h = 0; h < nf; h++) {
      P.adj_ptr[h + 1] = P.adj_ptr[h] + (int)adj[h].size();
      P.adj.insert(P.adj.end(), adj[h].begin(), adj[h].end());
    }
    for (int s = 0; s < P.nslots; s++) {
      const int r = P.slot_rc[2 * s], c = P.slot_rc[2 * s + 1];
      if (P.jpos[r] >= 0 && P.jpos[c] >= 0) { P.jj.push_back(s); P.jj.push_back(P.jpos[r]); P.jj.push_back(P.jpos[c]); }
    }
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  return P.nj > kPgoMaxJunctions ? SBM_ERR_UNSUPPORTED : SBM_OK;
}

static void pgo_plan_info(const PgoPlan& P, sbm_pgo_plan_info* o) {
  o->n_free = P.nfree; o->n_runs = P.nruns; o->n_junctions = P.nj; o->schur_size = 6 * P.nj; o->n_coupling = P.ncoupling;
  o->longest_run = P.longest; o->n_slots = P.nslots; o->max_junctions = kPgoMaxJunctions;
}

// ---- one optimisation on the device ------------------------------------------------------------------------------------------------
template <class T> static hipError_t upload(DevBuf& b, size_t& off, const std::vector<T>& v, hipStream_t s, T** out) {
  off = (off + 15) & ~(size_t)15;
  *out = (T*)((char*)b.p + off);
  const size_t n = v.size() * sizeof(T);
  off += n;
  return n ? hipMemcpyAsync(*out, v.data(), n, hipMemcpyHostToDevice, s) : hipSuccess;
}
static size_t padded(size_t n) { return (n + 15) & ~(size_t)15; }

struct PgoDev {   // where the pieces of one call lie in the handle's buffers
  int *vi, *vj, *hidx, *inc_ptr, *inc, *slot_ptr, *slot_edge, *sub, *jpos, *jidx, *vrun, *run_first, *run_len, *jj, *vfree, *adj_ptr, *adj, *slot_rc;
  double *poses, *meas, *info, *rec, *chi, *scal, *D, *bv, *Eoff, *Gs, *Ws, *Y, *x, *dotp, *S, *L, *xj, *rv;
};

// num iterations of HyperGraph::optimize on poses (sorted order, in place), then computeActiveErrors. edge_chi (may be null)
// receives the final per-edge chi2. Edges arrive as the plan's vi / vj with meas / info in edge order.
// The device form's arrays: poses in the caller's vertex order, measurements and information in edge order, and where the
// optimised poses go (ascending id order).
struct PgoDevIO { const double *poses, *meas, *info; double* poses_out; };

__global__ __launch_bounds__(64) void pgo_gather_poses_kernel(int nv, const int* __restrict__ order, const double* __restrict__ src,
                                                               double* __restrict__ dst) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= nv * 12) return;
  dst[t] = src[12 * (size_t)order[t / 12] + t % 12];
}

// With io the arrays are the caller's device memory (poses / meas / info are then ignored and may be null).
static int pgo_optimize(sbm_handle* h, const PgoPlan& P, int num, double* poses, const double* meas, const double* info,
                        double* err, double* edge_chi, const PgoDevIO* io = nullptr) {
  StageClock& clk = h->pgo.clock;
  hipStream_t s = h->stream;
  HIPCHK(h, clk.start(pgo_stages(), h->profiling != 0));
  const int nv = P.nv, ne = P.ne, nf = P.nfree, nj = P.nj;
  const size_t nints = padded(4 * (P.vi.size() + P.vj.size() + P.hidx.size() + P.inc_ptr.size() + P.inc.size() + P.slot_ptr.size() +
                                   P.slot_edge.size() + P.sub.size() + P.jpos.size() + P.jidx.size() + P.vrun.size() +
                                   P.run_first.size() + P.run_len.size() + P.jj.size() + P.vfree.size() + P.adj_ptr.size() + P.adj.size() +
                                   P.slot_rc.size() + P.order.size()) + 16 * 20);
  HIPCHK(h, h->pgo.graph.grow(nints + 8 * (12 * (size_t)nv + 48 * (size_t)ne), s));
  HIPCHK(h, h->pgo.edge.grow(8 * ((size_t)(kRec + 1) * std::max(ne, 1) + 8), s));
  const size_t nsys = 36 * (size_t)nf * 3 + 36 * (size_t)std::max(P.nslots, 1) + (size_t)nf * (6 + kPgoCols * 6 + 6 + 1 + 6) + 6 * (size_t)nj + 8;
  HIPCHK(h, h->pgo.sys.grow(8 * nsys, s));
  const size_t nS = blk(nj, 0);
  HIPCHK(h, h->pgo.schur.grow(8 * 2 * std::max(nS, (size_t)36), s));
  PgoDev d;
  size_t off = 0;
  DevBuf& gb = h->pgo.graph;
  HIPCHK(h, upload(gb, off, P.vi, s, &d.vi));
  HIPCHK(h, upload(gb, off, P.vj, s, &d.vj));
  HIPCHK(h, upload(gb, off, P.hidx, s, &d.hidx));
  HIPCHK(h, upload(gb, off, P.inc_ptr, s, &d.inc_ptr));
  HIPCHK(h, upload(gb, off, P.inc, s, &d.inc));
  HIPCHK(h, upload(gb, off, P.slot_ptr, s, &d.slot_ptr));
  HIPCHK(h, upload(gb, off, P.slot_edge, s, &d.slot_edge));
  HIPCHK(h, upload(gb, off, P.sub, s, &d.sub));
  HIPCHK(h, upload(gb, off, P.jpos, s, &d.jpos));
  HIPCHK(h, upload(gb, off, P.jidx, s, &d.jidx));
  HIPCHK(h, upload(gb, off, P.vrun, s, &d.vrun));
  HIPCHK(h, upload(gb, off, P.run_first, s, &d.run_first));
  HIPCHK(h, upload(gb, off, P.run_len, s, &d.run_len));
  HIPCHK(h, upload(gb, off, P.jj, s, &d.jj));
  HIPCHK(h, upload(gb, off, P.vfree, s, &d.vfree));
  HIPCHK(h, upload(gb, off, P.adj_ptr, s, &d.adj_ptr));
  HIPCHK(h, upload(gb, off, P.adj, s, &d.adj));
  HIPCHK(h, upload(gb, off, P.slot_rc, s, &d.slot_rc));
  int* d_order = nullptr;
  HIPCHK(h, upload(gb, off, P.order, s, &d_order));
  d.poses = (double*)((char*)gb.p + nints);
  d.meas = d.poses + 12 * (size_t)nv;
  d.info = d.meas + 12 * (size_t)ne;
  if (io) {
    hipLaunchKernelGGL(pgo_gather_poses_kernel, dim3((nv * 12 + 63) / 64), dim3(64), 0, s, nv, d_order, io->poses, d.poses);
    HIPCHK(h, hipGetLastError());
    if (ne) {
      HIPCHK(h, hipMemcpyAsync(d.meas, io->meas, 96 * (size_t)ne, hipMemcpyDeviceToDevice, s));
      HIPCHK(h, hipMemcpyAsync(d.info, io->info, 288 * (size_t)ne, hipMemcpyDeviceToDevice, s));
    }
  } else {
    HIPCHK(h, hipMemcpyAsync(d.poses, poses, 96 * (size_t)nv, hipMemcpyHostToDevice, s));
  }
  if (ne && !io) {
    HIPCHK(h, hipMemcpyAsync(d.meas, meas, 96 * (size_t)ne, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d.info, info, 288 * (size_t)ne, hipMemcpyHostToDevice, s));
  }
  d.scal = h->pgo.edge.as<double>();          // chi2, scaleLambda's sum, max_diag
  d.chi = d.scal + 8;
  d.rec = d.chi + std::max(ne, 1);
  d.D = h->pgo.sys.as<double>();
  d.Gs = d.D + 36 * (size_t)nf;
  d.Ws = d.Gs + 36 * (size_t)nf;
  d.Eoff = d.Ws + 36 * (size_t)nf;
  d.bv = d.Eoff + 36 * (size_t)std::max(P.nslots, 1);
  d.Y = d.bv + 6 * (size_t)nf;
  d.x = d.Y + (size_t)nf * kPgoCols * 6;
  d.dotp = d.x + 6 * (size_t)nf;
  d.xj = d.dotp + nf;
  d.rv = d.xj + 6 * (size_t)nj;
  d.S = h->pgo.schur.as<double>();
  d.L = d.S + std::max(nS, (size_t)36);
  HIPCHK(h, hipMemsetAsync(d.scal, 0, 64, s));
  h->pgo.dev = PgoDebug{};
  h->pgo.last = PgoLast{ne, nf, P.nslots, nj, P.nruns, 0, 0.0};
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
  if (io) HIPCHK(h, hipMemcpyAsync(io->poses_out, d.poses, 96 * (size_t)nv, hipMemcpyDeviceToDevice, s));
  else HIPCHK(h, hipMemcpyAsync(poses, d.poses, 96 * (size_t)nv, hipMemcpyDeviceToHost, s));
  if (edge_chi && ne) HIPCHK(h, hipMemcpyAsync(edge_chi, d.chi, 8 * (size_t)ne, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  *err = scal[0];
  h->pgo.dev = PgoDebug{d.rec, d.D, d.Eoff, d.bv, d.x};
  return SBM_OK;
}

// getConnectedGraph as written, on links in the caller's multimap order (keyed by `from`). Propagation in double.
struct PgoLinks { std::vector<int> from, to; std::vector<double> meas, info; };
static void pgo_connected(int from_id, const std::map<int, Rt>& in, const PgoLinks& lin, std::map<int, Rt>& out, std::vector<int>& kept) {
  out.clear(); kept.clear();
  std::multimap<int, int> bi, by_from;   // by_from: from -> link index, in order
  const int n = (int)lin.from.size();
  for (int k = 0; k < n; k++) {
    bi.insert({lin.from[k], lin.to[k]});
    bi.insert({lin.to[k], lin.from[k]});
    by_from.insert({lin.from[k], k});
  }
  auto find = [&](const std::multimap<int, int>& idx, int a, int b) {
    for (auto r = idx.equal_range(a); r.first != r.second; ++r.first)
      if (lin.to[r.first->second] == b) return r.first->second;
    for (auto r = idx.equal_range(b); r.first != r.second; ++r.first)
      if (lin.to[r.first->second] == a) return r.first->second;
    return -1;
  };
  std::multimap<int, int> kept_by_from;
  std::map<int, bool> pending;   // an ordered set
  pending[from_id] = true;
  while (!pending.empty()) {
    const int cur = pending.rbegin()->first;
    pending.erase(cur);
    if (out.empty()) out.insert({cur, in.find(cur)->second});
    for (auto r = bi.equal_range(cur); r.first != r.second; ++r.first) {
      const int to = r.first->second;
      const int k = find(by_from, cur, to);
      if (pending.count(to)) continue;
      if (!out.count(to)) {
        const Rt T = load_rt(&lin.meas[12 * (size_t)k]);
        out.insert({to, lin.from[k] == cur ? compose(out.at(cur), T) : compose(out.at(cur), inverse(T))});
        pending[to] = true;
      }
      if (find(kept_by_from, cur, to) < 0) kept_by_from.insert({lin.from[k], k});
    }
  }
  for (const auto& kv : kept_by_from) kept.push_back(kv.second);   // the out-multimap's order: by from, insertion order among equals
}

}  // namespace sbm

using namespace sbm;

extern "C" {

void sbm_pgo_params_default(sbm_pgo_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->num = 20;
  p->fixed_id = 1;
  p->coupling = SBM_PGO_COUPLING_REFERENCE;
  p->run_max = 64;
}

int sbm_pgo_params_check(const sbm_pgo_params* p, const sbm_pgo_graph* g) { return pgo_check(p, g); }

int sbm_pgo_plan(const sbm_pgo_params* p, const sbm_pgo_graph* g, sbm_pgo_plan_info* info, int32_t* vertex_run, int32_t* slot_rc,
                 uint8_t* edge_couples) {
  if (!info) return SBM_ERR_NULL;
  int st = pgo_check(p, g);
  if (st != SBM_OK) return st;
  PgoPlan P;
  st = pgo_make_plan(p, g, P);
  if (st != SBM_OK && st != SBM_ERR_UNSUPPORTED) return st;
  pgo_plan_info(P, info);
  if (vertex_run) std::copy(P.vrun.begin(), P.vrun.end(), vertex_run);
  if (slot_rc) std::copy(P.slot_rc.begin(), P.slot_rc.end(), slot_rc);
  if (edge_couples) std::copy(P.couples.begin(), P.couples.end(), edge_couples);
  return st;
}

int sbm_pgo_optimize(sbm_handle* h, const sbm_pgo_params* p, const sbm_pgo_graph* g, double* poses_out, double* err) {
  if (!h || !poses_out || !err) return SBM_ERR_NULL;
  int st = pgo_check(p, g);
  if (st != SBM_OK) return st;
  try {
    PgoPlan P;
    st = pgo_make_plan(p, g, P);
    if (st != SBM_OK) return st;
    std::vector<double> poses(12 * (size_t)P.nv);
    for (int i = 0; i < P.nv; i++) memcpy(&poses[12 * (size_t)i], g->poses + 12 * (size_t)P.order[i], 96);
    DeviceScope dscope(h->device);
    HIPCHK(h, dscope.enter());
    st = pgo_optimize(h, P, p->num, poses.data(), g->meas, g->info, err, nullptr);
    if (st != SBM_OK) return st;
    pgo_plan_info(P, &h->pgo.plan);
    memcpy(poses_out, poses.data(), 96 * (size_t)P.nv);
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  return SBM_OK;
}

int sbm_pgo_optimize_device(sbm_handle* h, const sbm_pgo_params* p, const sbm_pgo_graph* g, void* d_poses_out, double* err) {
  if (!h || !d_poses_out || !err) return SBM_ERR_NULL;
  int st = pgo_check(p, g, false);
  if (st != SBM_OK) return st;
  try {
    PgoPlan P;
    st = pgo_make_plan(p, g, P);
    if (st != SBM_OK) return st;
    DeviceScope dscope(h->device);
    HIPCHK(h, dscope.enter());
    const PgoDevIO io = {g->poses, g->meas, g->info, (double*)d_poses_out};
    st = pgo_optimize(h, P, p->num, nullptr, nullptr, nullptr, err, nullptr, &io);
    if (st != SBM_OK) return st;
    pgo_plan_info(P, &h->pgo.plan);
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  return SBM_OK;
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
      for (int k : kept) {
        sel.from.push_back(alive.from[k]);
        sel.to.push_back(alive.to[k]);
        sel.meas.insert(sel.meas.end(), &alive.meas[12 * (size_t)k], &alive.meas[12 * (size_t)k] + 12);
        sel.info.insert(sel.info.end(), &alive.info[36 * (size_t)k], &alive.info[36 * (size_t)k] + 36);
      }
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
      std::vector<double> poses(poses0), chi(sel.from.size() + 1);
      double e5;
      st = pgo_optimize(h, P, 5, poses.data(), sel.meas.data(), sel.info.data(), &e5, chi.data());
      if (st != SBM_OK) return st;
      int worst = -1;
      double werr = 0;
      for (size_t k = 0; k < sel.from.size(); k++) {
        const int a = sel.from[k], b = sel.to[k];
        if (a != b + 1 && b != a + 1 && chi[k] >= 10.0 && chi[k] > werr) { worst = (int)k; werr = chi[k]; }
      }
      if (worst < 0) {   // runOptimize from the re-propagated poses, not from the five-iteration result
        poses = poses0;
        st = pgo_optimize(h, P, p->num, poses.data(), sel.meas.data(), sel.info.data(), err, nullptr);
        if (st != SBM_OK) return st;
        pgo_plan_info(P, &h->pgo.plan);
        *n_out = (int32_t)ids.size();
        memcpy(ids_out, ids.data(), 4 * ids.size());
        memcpy(poses_out, poses.data(), 8 * poses.size());
        return SBM_OK;
      }
      const int a = sel.from[(size_t)worst], b = sel.to[(size_t)worst];
      if (*n_removed < removed_cap) { removed[2 * *n_removed] = a; removed[2 * *n_removed + 1] = b; }
      ++*n_removed;
      PgoLinks next;
      for (size_t k = 0; k < sel.from.size(); k++) {
        if (sel.from[k] == a && sel.to[k] == b) continue;   // every link with that (from, to)
        next.from.push_back(sel.from[k]);
        next.to.push_back(sel.to[k]);
        next.meas.insert(next.meas.end(), &sel.meas[12 * k], &sel.meas[12 * k] + 12);
        next.info.insert(next.info.end(), &sel.info[36 * k], &sel.info[36 * k] + 36);
      }
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
  if (!h->pgo.dev.rec) return SBM_ERR_UNSUPPORTED;
  const auto& L = h->pgo.last;
  const void* src = nullptr;
  size_t n = 0;
  switch (which) {
    case SBM_PGO_DEBUG_EDGES: src = h->pgo.dev.rec; n = 8 * (size_t)kRec * L.ne; break;
    case SBM_PGO_DEBUG_DIAG: src = h->pgo.dev.D; n = 288 * (size_t)L.nfree; break;
    case SBM_PGO_DEBUG_OFFDIAG: src = h->pgo.dev.Eoff; n = 288 * (size_t)L.nslots; break;
    case SBM_PGO_DEBUG_B: src = h->pgo.dev.bv; n = 48 * (size_t)L.nfree; break;
    case SBM_PGO_DEBUG_X: src = h->pgo.dev.x; n = 48 * (size_t)L.nfree; break;
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
