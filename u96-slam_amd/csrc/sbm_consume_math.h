// sbm_consume_math.h -- the reference's per-point arithmetic that the consumers of the disparity map share (sbm_consume.hip,
// the occupancy family through sbm_occ.h): projectDisparityTo3D, isFinite and transformPoint (Stereo.cpp:157-199). Internal, gfx950 only.
// Types per operation as in the C++ source, and never a contracted multiply-add: the including files are built with
// -ffp-contract=off or carry the pragma, and the functions below carry it too.
#pragma once
#include "sbm_common.h"

namespace sbm {

struct Pt3 { float x, y, z; };

__device__ __forceinline__ Pt3 nan3() {
  const float q = __builtin_nanf("");
  return Pt3{q, q, q};
}

// Stereo.cpp:157-182
__device__ __forceinline__ Pt3 project_disparity(float px, float py, float disp, const sbm_stereo_model& m) {
#pragma clang fp contract(off)
  if (!(disp > 0.0f)) return nan3();
  const float c = (float)(m.cx_r - m.cx_l);
  const float dc = disp + c;                                                    // float + float
  const float Wx = (float)((m.Tx_l / m.fx_l - m.Tx_r / m.fx_r) / (double)dc);
  const float Wy = (float)((m.Tx_l / m.fy_l - m.Tx_r / m.fy_r) / (double)dc);
  Pt3 p;
  p.x = (float)(((double)px - m.cx_l) * (double)Wx);
  p.y = (float)(((double)py - m.cy_l) * (double)Wy);
  p.z = (float)(m.fx_l * (double)Wx);
  return p;
}

__device__ __forceinline__ bool finite3(const Pt3& p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// Stereo.cpp:189-199 (float arithmetic, left-to-right sums)
__device__ __forceinline__ Pt3 transform_point(const Pt3& p, const float* t) {
#pragma clang fp contract(off)
  Pt3 r;
  r.x = t[0] * p.x + t[1] * p.y + t[2] * p.z + t[3];
  r.y = t[4] * p.x + t[5] * p.y + t[6] * p.z + t[7];
  r.z = t[8] * p.x + t[9] * p.y + t[10] * p.z + t[11];
  return r;
}

}  // namespace sbm
