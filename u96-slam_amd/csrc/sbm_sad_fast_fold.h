// sbm_sad_fast_fold.h -- the FOLDED leftover strip of the interior SAD kernel: the last plain strip of a 128-disparity, 15-window
// launch when it has at most FoldLds::NV = 22 columns left (KITTI: 1 101 interior columns = 6 x 180 + 21). Included by
// sbm_sad_fast_kernel.h. gfx950 only.
//
// The plain strip (sbm_sad_fast_strip.h) runs the whole 128-disparity row on such a remainder with 33 of its 64 lanes doing
// anything useful. Here the wavefront is folded over the disparity range instead: lane = (h, i), h = lane >> 5, i = lane & 31;
// both halves sit on the SAME columns cbase + i, the lower half carries buffer indices 0..63, the upper half 64..127 -- 16
// quads per lane instead of 32, so the subtractions of the leaving row, the exchange, the winner search, the deficit pass and
// the neighbour tree run at half length.
//   sums      = 5-column vertical sums V5(c) = columns c..c+4 at lane stride 1 and a 3-term window S(c + 7) = V5(c) + V5(c + 5)
//               + V5(c + 10): a halo of 10 lanes, 22 of 32 columns produce. V5 is two v_mqsad_pk_u16_u8 per quad and row:
//               pattern L[c..c+3] against the staged dword pair (base + 4q, base + 4q + 4), then the one-byte pattern L[c+4]
//               (the other bytes 0: masked) against (base + 4q + 4, base + 4q + 8), into the same register. base = i + 64 h:
//               the window of buffer index d starts at byte c + d, so the upper half reads 64 bytes further into the same
//               staged right piece (highest slot 31 + 64 + 60 + 8 = 163 of the 192 the plain strip stages as well).
//   exchange  = as the plain strip's direct sum with partners at lane + 5 and lane + 10, each half in its own entries (entry =
//               lane): one publish, two reads, one three-operand add per entry. Tag carriers (FastTag): (i / 5) % 3 == 0.
//   tail      = what the cooperating wavefronts (NWAVES > 1) do through LDS and two barriers, between the two HALVES through
//               v_permlane32_swap: winner = min over the halves of (sum << 16 | index + 64 h) (equal sums: the smaller index
//               is the smaller key); deficit sums added per 16-bit half (saturating); S[mind -+ 1] from the half that owns the
//               index. Both halves then hold the same verdict; the lower half stores.
//   hand-off  = as the plain strip, in the first 16 x 512 + 256 bytes of the strip's slot: the segment plan stays uniform.
// Everything else -- staging, the order of the row loop, the late stores -- is the plain strip's; see there for the reasons.
#pragma once
#include "sbm_sad_fast_core.h"

namespace sbm {

__device__ __forceinline__ void sad_fast_strip_fold(const FastArgs& a, unsigned char* __restrict__ const b0c, unsigned char* __restrict__ const b1c,
                                                    const int cbase, const int segi, const int pair, const int strip) {
  using D = FoldLds;
  typedef __attribute__((address_space(3))) void* lds_vptr;
  constexpr int NQ = D::NQ;             // disparity quads of a lane (one u64 accumulator each)
  constexpr int NR = 2 * NQ;            // packed pair registers
  constexpr int NIT = D::NSLOT / 64;
  constexpr int WSZ = D::PW * D::NTERM, W2 = WSZ / 2;
  constexpr int KS = D::KS, XCH = D::XCH, XS = D::XS;
  constexpr int SLOT_B = FastHandoff<D::NDW, 1, true>::SLOT_B;   // the strip's slot is the plain strip's; the first NQ quads and 256 bytes are used

  const int lane = threadIdx.x & 63;
  const unsigned lane_u = (unsigned)lane;
  const int col = lane & 31;                            // i: this lane's column within the strip
  const u32 half = lane_u >> 5;                         // h: which 64 buffer indices
  const int c = cbase + col;                            // this lane's column (relative to lofs): V5 covers c..c+4
  const int xc = c + W2;                                // centre column this lane produces
  const bool produces = col < D::NV && xc >= a.xc0 && xc < a.xc1;
  const int ys = a.segrow[segi];
  const int ye = a.segrow[segi + 1];
  const uint8_t* pl = a.pf_l + (size_t)pair * a.plane + a.padl + a.lofs + cbase;
  const uint8_t* pr = a.pf_r + (size_t)pair * a.plane + a.padl + a.rofs + cbase;
  const __amdgpu_buffer_rsrc_t rs_l = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(pl), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(pr), 0, 0x7fffffff, 0x00020000);
  uint4* const b0 = reinterpret_cast<uint4*>(b0c);
  uint4* const b1 = reinterpret_cast<uint4*>(b1c);
  uint4* const xq0 = b0;                                // the exchange area: [XS] quad pairs, then [XS] texture column sums
  u32* const xt0 = reinterpret_cast<u32*>(xq0 + (XCH / 2) * XS);
  const u32 capw = (u32)a.capb * 0x01010101u;

  // vertical sums of this lane's 64 buffer indices, accumulated in place; the carrier lanes start at their registers' tags
  u64 VB[NQ];
  {
    const u32 unit = ((unsigned)col / (unsigned)KS) % (unsigned)D::NTERM == 0u ? FastTag<WSZ>::tag_unit(a.pfshift) : 0u;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const u32 tq = (u32)((2 * q) / (NR / FastTag<WSZ>::NGRP)) * unit;
      VB[q] = __builtin_bit_cast(u64, make_uint2(tq, tq));
    }
  }
  u32 Vt = 0;  // texture: window-row sum of the 5-column |L - cap| (the same in both halves)

  auto pat_of = [](uint4* const buf) { return reinterpret_cast<u32*>(reinterpret_cast<unsigned char*>(buf) + D::PAT_OFS); };
  auto stage = [&](const int y, uint4* const buf) {
    const int rowoff = __builtin_amdgcn_readfirstlane(y * a.pitch);
#pragma unroll
    for (int it = 0; it < NIT; it++)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_r, (lds_vptr)(reinterpret_cast<u32*>(buf) + 64 * it), 4, (int)lane_u, rowoff + 64 * it, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_l, (lds_vptr)pat_of(buf), 4, (int)lane_u, rowoff, 0, 0);
  };
  auto landed = [] {
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto reads_done = [] {
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
  };
  auto published = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  // the staged row in `buf` enters (leave == false) or leaves the vertical sums
  auto apply = [&](uint4* const buf, const bool leave) {
    const u32 pat4 = pat_of(buf)[col];               // L[c..c+3]
    const u32 pat1 = pat_of(buf)[col + 4] & 0xffu;   // L[c+4]; the other bytes 0 -> masked by mqsad
    const u32 tv = __builtin_amdgcn_sad_u8(pat1 | (capw & ~0xffu), capw, __builtin_amdgcn_sad_u8(pat4, capw, 0u));
    // dword slot p = bytes p..p+3 of the right piece: quad q of this half reads the slots base + 4q, + 4, + 8
    const u32* const win4 = reinterpret_cast<const u32*>(buf) + col + 64 * (int)half;
    u32 lo[NQ], mi[NQ], mj[NQ], hi[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) { lo[q] = win4[4 * q]; mi[q] = win4[4 * q + 4]; }
#pragma unroll
    for (int q = 0; q < NQ; q++) { mj[q] = win4[4 * q + 4]; hi[q] = win4[4 * q + 8]; }
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const u64 w0 = ((u64)mi[q] << 32) | lo[q], w1 = ((u64)hi[q] << 32) | mj[q];
      if (!leave) {
        asm("v_mqsad_pk_u16_u8 %0, %1, %2, %0" : "+v"(VB[q]) : "v"(w0), "v"(pat4));
        asm("v_mqsad_pk_u16_u8 %0, %1, %2, %0" : "+v"(VB[q]) : "v"(w1), "v"(pat1));
      } else {
        const u64 t0 = __builtin_amdgcn_mqsad_pk_u16_u8(w0, pat4, 0ull);
        const uint2 tt = __builtin_bit_cast(uint2, __builtin_amdgcn_mqsad_pk_u16_u8(w1, pat1, t0));
        uint2 vb = __builtin_bit_cast(uint2, VB[q]);
        vb.x -= tt.x;                                         // no u16 lane borrows: every partial sum is exact
        vb.y -= tt.y;
        asm("" : "+v"(vb.x), "+v"(vb.y));                     // (two 32-bit subtractions, not a 64-bit one with a carry chain)
        VB[q] = __builtin_bit_cast(u64, vb);
      }
    }
    Vt = leave ? Vt - tv : Vt + tv;
  };

  // the sums this segment starts from: taken over from the segment above where they are there, else primed (sad_fast_strip_dma)
  const size_t ho_set = (size_t)a.npairs * a.strips;
  const size_t ho_slots = (size_t)__builtin_popcountll(a.ho_link) * ho_set;
  auto ho_slot = [&](const int k) { return (size_t)__builtin_popcountll(a.ho_link & ((1ull << k) - 1)) * ho_set + (size_t)pair * a.strips + strip; };
  auto ho_rsrc = [&](const size_t slot) {
    unsigned char* const p = reinterpret_cast<unsigned char*>(a.ho) + ((2 * ho_slots * sizeof(u32) + 255) & ~(size_t)255) + slot * SLOT_B;
    return __builtin_amdgcn_make_buffer_rsrc(p, 0, NQ * 512 + 256, 0x00020000);
  };
  bool take = false;
  if ((a.ho_link >> segi) & 1) {
    const size_t from = ho_slot(segi);
    take = __builtin_amdgcn_readfirstlane(__hip_atomic_load(a.ho + from, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == a.ho_epoch;
    if (take) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      const __amdgpu_buffer_rsrc_t rs_h = ho_rsrc(from);
#pragma unroll
      for (int q = 0; q < NQ; q++) VB[q] = __builtin_bit_cast(u64, __builtin_amdgcn_raw_buffer_load_b64(rs_h, (int)(8 * lane_u), 512 * q, kHandoffAux));
      Vt = __builtin_amdgcn_raw_buffer_load_b32(rs_h, (int)(4 * lane_u), 512 * NQ, kHandoffAux);
      if (lane == 0) a.ho[ho_slots + from] = a.ho_epoch;   // "taken"
      stage(ys + W2, b0);   // the first output row's entering row
    }
  }
  if (!take) {
    stage(ys - W2, b0);
    for (int i = 0; i < 2 * W2; i += 2) {
      landed();
      stage(ys - W2 + i + 1, b1);
      apply(b0, false);
      landed();
      stage(ys - W2 + i + 2, b0);
      apply(b1, false);
    }
  }
  const __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(a.disp + (size_t)pair * a.W * a.H, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_c = __builtin_amdgcn_make_buffer_rsrc(a.cost + (size_t)pair * a.W * a.H, 0, 0x7fffffff, 0x00020000);
  const int ocol_u = __builtin_amdgcn_readfirstlane(2 * (a.lofs + cbase + W2));
  const bool stores = produces && half == 0u;   // both halves hold the verdict; the lower one stores it, one row late
  u32 res_prev = 0xffff0000u;
  auto flush = [&](const int yrow) {
    if (stores) {
      const int orow_prev = __builtin_amdgcn_readfirstlane(2 * yrow * a.W) + ocol_u;
      const int ocol = 2 * col;
      if (a.cost) __builtin_amdgcn_raw_buffer_store_b16((short)(res_prev >> 16), rs_c, ocol, orow_prev, 0);
      __builtin_amdgcn_raw_buffer_store_b16((short)res_prev, rs_d, ocol, orow_prev, 0);
    }
  };
  for (int y = ys; y < ye; y++) {
    landed();
    if (y > ys) {
      flush(y - 1);
      apply(b1, true);
    }
    reads_done();
    stage(y - W2, b1);
    apply(b0, false);

    __builtin_amdgcn_s_setprio(kFastPrioExchange);
    // ---- horizontal window across lanes: S(c + 7) = V5(c) + V5(c + 5) + V5(c + 10), a chunk of XCH quads at a time. Lanes with
    // i >= NV read entries of the other half or entries nobody wrote: their sums are garbage and never stored. Partner entries
    // are addressed through an opaque copy of the lane index (sad_fast_strip_dma says why).
    u32 S[NR];
    unsigned long long tex_ok = 0;
    u32 lx = lane_u;
    asm volatile("" : "+v"(lx));
#pragma unroll
    for (int q0 = 0; q0 < NQ; q0 += XCH) {
      const bool tex_now = q0 == 0;
      const uint2 v0 = __builtin_bit_cast(uint2, VB[q0]), v1 = __builtin_bit_cast(uint2, VB[q0 + 1]);
      xq0[lane] = make_uint4(v0.x, v0.y, v1.x, v1.y);
      if (tex_now) xt0[lane] = Vt;
      published();
      const uint4 r1 = xq0[lx + KS], r2 = xq0[lx + 2 * KS];
      S[2 * q0 + 0] = v0.x + r1.x + r2.x;   // packed u16 pairs: no carries, every sum stays below 65535
      S[2 * q0 + 1] = v0.y + r1.y + r2.y;
      S[2 * q0 + 2] = v1.x + r1.z + r2.z;
      S[2 * q0 + 3] = v1.y + r1.w + r2.w;
      if (tex_now) {
        const u32 tA = Vt + xt0[lx + KS] + xt0[lx + 2 * KS];
        tex_ok = __ballot((int)tA >= a.tex);
      }
      __builtin_amdgcn_wave_barrier();
    }
    reads_done();
    stage(min(y + 1 + W2, a.H - 1), b0);
    __builtin_amdgcn_s_setprio(0);

    // ---- WTA: each half's first minimum over its 64 indices, then the smaller key of the two halves -------------------------
    u32 best = fast_first_min<NR, WSZ>(S, a.pfshift) + 64u * half;
    {
      const auto r = __builtin_amdgcn_permlane32_swap(best, best, false, false);   // r[0]: the lower half's, r[1]: the upper half's
      best = min(r[0], r[1]);
    }
    const int minsad = (int)(best >> 16), mind = (int)(best & 0xffffu);

    // ---- uniqueness (part 1): each half's saturating deficit sums, added per 16-bit half (even / odd indices: 64 is even) ------
    u32 acc = 0, T = 0;
    if (a.uniq > 0) {
      T = fast_uniq_threshold(minsad, a.uniq, a.pfshift);
      acc = fast_deficits<NR, WSZ>(S, T, a.uniq_plain, a.pfshift);
      const auto r = __builtin_amdgcn_permlane32_swap(acc, acc, false, false);
      acc = pk_add_sat(r[0], r[1]);
    }

    // ---- neighbours S[mind-1], S[mind+1] (mirrored at the ends): each from the half that owns the index -----------------------
    const int in_ = mind > 0 ? mind - 1 : 1;
    const int ip_ = mind < a.nd - 1 ? mind + 1 : a.nd - 2;
    const int d0 = 64 * (int)half;
    const int ln = min(max(in_ - d0, 0), 63), lp = min(max(ip_ - d0, 0), 63);  // local (clamped) indices
    int nn, pp;
    {
      u32 X[NQ];
      const u32 lnp = (u32)ln | ((u32)lp << 16);
      fast_neighbours_quads<NQ>(S, lnp, X);
      const u32 X0 = fast_neighbours_tree<NQ>(X, lnp) & ~(((1u << a.pfshift) - 1u) * 0x00010001u);   // (without the tags)
      const auto r = __builtin_amdgcn_permlane32_swap(X0, X0, false, false);
      nn = (int)((in_ >= 64 ? r[1] : r[0]) & 0xffffu);
      pp = (int)((ip_ >= 64 ? r[1] : r[0]) >> 16);
    }

    bool ok = __builtin_amdgcn_inverse_ballot_w64(tex_ok);
    // ---- uniqueness (part 2) -------------------------------------------------------------------------------------------------
    if (a.uniq > 0) ok = ok && fast_unique(acc & 0xffffu, acc >> 16, T, minsad, mind, nn, pp, a.nd);
    if (stores) {
      int out = a.filtered, cst = -1;
      if (ok) {
        out = fast_subpixel(nn, pp, minsad, mind, a.nd, a.mindisp);
        if (a.cost) cst = minsad >> a.pfshift;
      }
      res_prev = ((u32)out & 0xffffu) | ((u32)cst << 16);
    }
  }
  flush(ye - 1);   // the segment's last row
  // leave the sums for the next segment of this (pair, strip): the primed state of a segment that starts at ye (sad_fast_strip_dma)
  if (segi + 1 < a.nseg && ((a.ho_link >> (segi + 1)) & 1)) {
    landed();
    apply(b1, true);
    const size_t ho_mine = ho_slot(segi + 1);
    const __amdgpu_buffer_rsrc_t rs_h = ho_rsrc(ho_mine);
#pragma unroll
    for (int q = 0; q < NQ; q++) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, VB[q]), rs_h, (int)(8 * lane_u), 512 * q, kHandoffAux);
    __builtin_amdgcn_raw_buffer_store_b32(Vt, rs_h, (int)(4 * lane_u), 512 * NQ, kHandoffAux);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_store(a.ho + ho_mine, a.ho_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace sbm
