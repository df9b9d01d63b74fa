// sbm_sad_fast.hip -- the hot kernel: windowed SAD over the disparity range + WTA + texture + uniqueness +
// sub-pixel, for the interior (unclamped) columns.  gfx950 / CDNA4 only.
//
// Device counterpart of findStereoCorrespondenceBM (OpenCV calib3d stereobm.cpp) reached from
// src/slam/src/core/main.cpp:215.  In-tree hardware twins: src/dvp/rtl/bm_calc_sad.v:391-605 (34-lane abs-diff,
// vertical running sums, horizontal running SAD), bm_calc_det.v:124-426 (WTA tree), bm_calc_frac.v (sub-pixel).
//
// Mapping (a workgroup = NWAVES cooperating wavefronts over the SAME 64 columns; wavefront k owns disparities
// [NDW*k, NDW*k+NDW); two barriers per row where NWAVES > 1, none otherwise):
//   lane      = one image column c (64 consecutive columns per workgroup), marching down a row segment
//   registers = V[d]: for every disparity the sum over the w window rows of the 3-column SAD
//               H3(c,y,d) = sum_{i<3} |Lp[y][c+i] - Rp[y][c+i-D]|, packed 4 x u16 per VGPR pair.
//               One v_mqsad_pk_u16_u8 produces H3 for 4 consecutive disparities AND accumulates (pattern = 3 left
//               bytes + a zero byte, which the instruction masks; sliding 8-byte window = right bytes).
//               Entering row: V = mqsad(R, L, V), accumulated IN PLACE (vdst == src2: right on gfx950, checked by a device
//               self-test; a device that fails it takes the sliding-sum kernel).  Leaving row: V -= mqsad(R, L, 0).
//   LDS       = the right row piece of the wavefront, staged by LDS-direct loads (buffer_load_dword ... lds: no staging
//               registers) into a 4x-expanded layout -- dword slot p holds bytes p..p+3, so a quad's 8-byte window is the
//               dword pair (4q, 4q+4) behind the lane's slot, one conflict-free ds_read2_b32 (sad_fast_strip_dma,
//               sbm_sad_fast_strip.h).
//   exchange  = horizontal window: S(c + w/2) = sum_k V(c + 3k), k < w/3: lanes publish V to LDS ([quad pair][lane],
//               16 B entries) and read the shifted copies back; from 7 terms on in two levels (HPlan: T = a few V,
//               published again, window = a few T + the remaining V). Lanes whose partners fall outside the wavefront
//               produce nothing and are recomputed by the next strip.
//   WTA       = in registers: min over (S << 16 | d) keys (first d wins ties, as cv's strict '<' scan; a tagged packed
//               search on pre-scaled planes where the sums leave bits free), uniqueness by a saturating deficit sum,
//               S[mind +- 1] by a v_perm_b32 selection tree; per-wavefront results merged through LDS, one wavefront
//               (alternating per row) finishes and stores.
// Column stride (template parameter CS, windows that are multiples of 3): with CS = 3 lane i takes column base + 3 i, so the
// partners of the horizontal window V(c), V(c+3), ... are the NEXT LANES and only NTERM - 1 lanes of a wavefront produce
// nothing (w 15: 60 of 64 lanes useful instead of 52; w 21: 58 instead of 46). Three such wavefronts (bases b, b+1, b+2)
// tile 3 * (65 - NTERM) contiguous columns; they are ordinary, independent strips. The right row piece a wavefront stages
// grows from 64 + nd to 190 + nd bytes (window reads at a lane stride of 48 bytes: still conflict-free), nothing else
// changes. Columns left over by the last full triple take CS = 1 strips -- both bodies live in one kernel, chosen by a
// workgroup-uniform branch on the strip index.
// Windows that are not multiples of 3 use 1-column sums (template parameter PW = 1: single-byte pattern, w-1 partners).
// Envelope (sad_fast_supported(); everything else, and everything on a device without the in-place accumulate, takes the
// sliding-sum kernel, sbm_sad_wide.hip): odd w in 5..31, nd <= 512, w*w*2*cap <= 65534 (16-bit sums),
// 2*(maxS*uniq/100+1) < 65535, valid-ROI rows inside [w/2, H-w/2).
//
// Source layout: sbm_sad_fast_core.h (arguments, LDS carve-up, exchange plan, the per-row tail: winner search / uniqueness /
// neighbours / sub-pixel), sbm_sad_fast_strip.h (the strip), sbm_sad_border_wave.h (the clamped border columns, extra wavefronts
// of the same launch), sbm_sad_fast_kernel.h (kernel + layout choice), and this file: the host side -- envelope, device
// self-test of the in-place accumulate, the launch's part of the call's plan (sad_fast_plan: strips, row segments, split; launch_t
// in sbm_sad_fast_kernel.h adds what depends on the instantiation) and the planned launch -- plus the kernels of the windows 15 and 21. The ~270
// instantiations compile as four translation units side by side (this one, sbm_sad_fast_pw1 / _pw2 / _pw3.hip: the other windows).
#include <string.h>

#include "sbm_sad_fast_kernel.h"

namespace sbm {

// Device check behind the in-place accumulate: v_mqsad_pk_u16_u8 with vdst == src2 against the compiler's
// non-aliased form, pseudo-random operands, single instructions and dependent chains (tools/ubench/mqsad_alias.hip
// is the long version); three short launches, once per device and process.
__global__ void __launch_bounds__(256) mqsad_inplace_selftest_kernel(unsigned* bad) {
  unsigned long long st = (unsigned long long)(blockIdx.x * 256 + threadIdx.x) * 0x9E3779B97F4A7C15ull + 88172645463325252ull;
  auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
  unsigned nbad = 0;
  for (int it = 0; it < 64; it++) {
    unsigned long long accA[4], accR[4], win[4];
    const unsigned pat = (unsigned)rnd() & ((it & 1) ? 0x00ffffffu : 0x000000ffu);
#pragma unroll
    for (int q = 0; q < 4; q++) { accA[q] = accR[q] = rnd() & 0x3fff3fff3fff3fffull; win[q] = rnd(); }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        accR[q] = __builtin_amdgcn_mqsad_pk_u16_u8(win[(q + r) & 3], pat, accR[q]);
        asm volatile("v_mqsad_pk_u16_u8 %0, %1, %2, %0" : "+v"(accA[q]) : "v"(win[(q + r) & 3]), "v"(pat));
      }
#pragma unroll
    for (int q = 0; q < 4; q++) nbad += accA[q] != accR[q];
  }
  if (nbad) atomicAdd(bad, nbad);
  atomicAdd(bad + 1, 1u);   // "this workgroup's thread ran": a launch that never executed must not read as a pass
}

// The check is launched at three occupancies -- 1, 4 and 8 wavefronts per SIMD chip-wide -- and passes only if every thread of
// every launch reported in and none saw a difference. A check that ran is cached per device for the process (under a mutex:
// handles may be created and used from several threads); one that could not run -- any of its HIP calls failed -- caches
// nothing and returns that call's error, so the next call runs it again. SBM_FAST_INPLACE=0 (read once) reports unavailable.
hipError_t mqsad_inplace_ok(hipStream_t s, bool* ok) {
  static const bool forced_off = env_switch("SBM_FAST_INPLACE", 1) == 0;
  static std::mutex mu;
  static signed char known[64];   // per device: 0 not run yet, 1 passed, -1 ran and mismatched
  *ok = false;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess || forced_off || dev < 0 || dev >= 64) return e;
  std::lock_guard<std::mutex> lock(mu);
  if (!known[dev]) {
    unsigned* d = nullptr;
    if ((e = hipMalloc(&d, 8)) != hipSuccess) return e;
    bool pass = true;
    const unsigned grids[3] = {256u, 1024u, 2048u};   // x 256 threads = 4 wavefronts per workgroup
    for (int k = 0; k < 3 && pass && e == hipSuccess; k++) {
      unsigned h[2] = {1u, 0u};
      e = hipMemsetAsync(d, 0, 8, s);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(mqsad_inplace_selftest_kernel, dim3(grids[k]), dim3(256), 0, s, d);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipMemcpyAsync(h, d, 8, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      pass = h[0] == 0u && h[1] == grids[k] * 256u;
    }
    const hipError_t ef = hipFree(d);
    if (e == hipSuccess) e = ef;
    if (e != hipSuccess) return e;
    known[dev] = pass ? 1 : -1;
  }
  *ok = known[dev] > 0;
  return hipSuccess;
}

// Pre-scaled planes for the tagged winner search: (value << sh) + 1 must fit a byte and (maxS << sh) + tag a packed half;
// the uniqueness envelope is the one of sad_fast_supported() on the scaled sums. SBM_FAST_PFSHIFT=0 turns it off, =1 limits
// it to one tag bit.
int sad_fast_pfshift(const Geom& g) {
  static const int env = env_switch("SBM_FAST_PFSHIFT", 2);
  if (env <= 0 || !sad_fast_supported(g)) return 0;
  const long maxs = (long)g.wsz * g.wsz * 2 * g.cap;
  // the kernels hold one tagged variant each: two tag bits (4 v + 1) for windows up to 15, one (2 v + 1) above
  const int sh = std::min(env, g.wsz <= 15 ? 2 : 1);
  const long f = 1L << sh;
  if (f * 2 * g.cap + 1 > 255) return 0;
  if (f * maxs + (f - 1) > 65535) return 0;
  if (2 * (f * (maxs * g.uniq / 100 + 1)) >= 65535) return 0;
  if ((long)g.tex * f > 0x3fffffff) return 0;
  return sh == (g.wsz <= 15 ? 2 : 1) ? sh : 0;
}

bool sad_fast_borders_in_launch(const Geom& g) { return g.nd <= 256; }

bool sad_fast_supported(const Geom& g) {
  if (g.wsz < 5 || g.wsz > 31) return false;   // every odd window 5..31: multiples of 3 with 3-column sums, the rest 1-column
  // up to 512 disparities: beyond 256 three / four cooperating 128-disparity wavefronts, whose border columns come from the
  // sliding-sum kernel (sbm_sad_wide.hip) in launches of their own
  if (g.nd > kFastNdMax) return false;
  const long maxs = (long)g.wsz * g.wsz * 2 * g.cap;
  if (maxs > 65534) return false;
  if (2 * (maxs * g.uniq / 100 + 1) >= 65535) return false;
  if (g.row0 < g.w2 || g.row1 > g.H - g.w2 || g.row1 <= g.row0) return false;
  if ((long)g.plane * 4 >= (1L << 31)) return false;   // a border wavefront reaches up to 4 pairs through 32-bit offsets
  const int xhi = std::min(g.W - g.lofs - 1, g.W - g.rofs - g.nd);  // last unclamped window column
  if (xhi - g.w2 + 1 <= g.w2) return false;
  return true;
}

// The window dispatch, for the plan (a == nullptr: launch_t fills it) and for the launch alike: the kernels of the windows 15 and
// 21 are here, the others in sbm_sad_fast_pw1 / _pw2 / _pw3.hip.
static hipError_t sad_fast_dispatch(BmPlan& pl, const FastArgs* a, hipStream_t s) {
  switch (pl.g.wsz) {
    case 15: return launch_nd<5, 3>(pl, a, s);
    case 21: return launch_nd<7, 3>(pl, a, s);
    default: return launch_sad_fast_pw1(pl, a, s);
  }
}

// SBM_FAST_HANDOFF, read per call (the GPU tests flip it): 1 (default) a row segment takes the vertical sums its predecessor
// left, if they are there when it starts; 0 every segment primes; 2 the segments go out as launches of their own, top to bottom,
// so that every hand-off is taken (for the tests of that path: it costs nseg launches).
static int fast_handoff_mode() { return std::max(0, std::min(2, env_switch("SBM_FAST_HANDOFF", 1))); }

// workgroups of a lone wavefront (up to 128 disparities) that the chip holds at once
static int fast_slots(int nd) { return nd <= 64 ? 4096 : 3072; }

// step of the first round's lengths (sad_fast_plan), as a share of a regular segment
constexpr double kFirstRoundStep = 0.10, kFirstRoundSpan = 0.40;

// Dispatch order of the row segments: at[p] = the segment whose per_seg workgroups (one per pair and strip) are dispatch
// position p of the grid, behind the border jobs. Returns the stride D of the order, nseg where it is the identity.
//
// Segment k + 1 finds the sums of segment k only if k has FINISHED when k + 1 is dispatched, and nothing may wait. Workgroups
// start in id order, each as a slot of the chip frees up: id j starts when j - slots + 1 workgroups have finished. With the
// segments in their natural order k + 1 lies per_seg ids behind k -- KITTI x 64: 1 216 chains per segment set against 3 072 slots
// -- so both run in the same round and no hand-off is ever taken. Put them D positions apart instead, D * per_seg >= slots + per_seg:
// position p + D then starts only when (p + 1) * per_seg workgroups have finished, and those are the sets of the positions 0 .. p as
// long as the sets finish in dispatch order -- a whole set's worth of finished workgroups lies between the predecessor's last one
// and the successor's first, so jitter inside a set does not matter. (One position less, D * per_seg >= slots, makes the
// successors start on the slots their own predecessors' set frees: a coin toss for the first of them.) Sets finish in dispatch
// order once the launch is past its first round; the first round's sets all start together, which is why sad_fast_plan gives
// them increasing lengths.
// So D = ceil(slots / per_seg) + 1, the positions p, p + D, p + 2 D, ... hold consecutive segments (a chain), and the chains follow
// each other: KITTI x 64, 8 segments, D = 4: positions 0..7 hold segments 0 2 4 6 1 3 5 7 -- segments 1, 3, 5, 7 take over, 4 of 8
// prime instead of 8. The positions D .. nseg-1 are the ones that take over, and they are the last ones: the tapered, short
// segments, which pay the largest priming share, are among them, and the launch still ends on short workgroups. The order
// within a set -- pairs over XCDs -- is untouched. A launch of fewer than D + 1 segments keeps the natural order and primes.
static int fast_segment_order(int nseg, long per_seg, int slots, int nd, unsigned char* at) {
  for (int k = 0; k < 64; k++) at[k] = (unsigned char)k;
  if (fast_handoff_mode() != 1 || nd > 128) return nseg;
  const long D = (slots + per_seg - 1) / per_seg + 1;
  if (D >= nseg) return nseg;
  int base = 0;
  for (int r = 0; r < (int)D; r++)
    for (int p = r; p < nseg; p += (int)D) at[p] = (unsigned char)base++;
  return (int)D;
}

// Scratch of the hand-off: per LINKED segment (one that may take its sums over: the segments behind the first D dispatch
// positions, every later segment in mode 2), pair and strip a ready word and a taken word, then (256-byte aligned) a slot of the
// sums -- the sets of slots in segment order, as sad_fast_strip_dma numbers them. A segment whose successor cannot take over holds
// no slot. Beyond kHandoffMaxBytes a call primes instead.
constexpr size_t kHandoffMaxBytes = (size_t)1 << 30;
static size_t fast_handoff_size(long linked, long per_seg, int ndw, size_t* flag_bytes) {
  const size_t slots = (size_t)linked * per_seg;
  *flag_bytes = (2 * slots * sizeof(u32) + 255) & ~(size_t)255;
  return *flag_bytes + slots * ((size_t)(ndw / 4) * 512 + 256);
}

// The row segments of a launch whose later segments take their sums over -- where fast_handoff_links() links them: a lone
// wavefront with an exact disparity count (32, 64, 128 disparities, not split), SBM_FAST_HANDOFF=1 and a dispatch order of
// stride D < nseg for sad_fast_plan's own count nseg. Every other launch keeps sad_fast_plan's rule (returns 0); otherwise
// the count, with len[p] the rows of DISPATCH POSITION p.
//
// Two prices. A segment at a position below D primes: w - 1 rows at 0.2 of a row each, as sad_fast_plan charges. A segment at a
// later position pays one hand-off -- the extra leaving row, the slot's store and load, the wait in front of the ready word:
// kHandoffRows = 0.7 of a row. Measured, KITTI x64 (1242x375 nd 128 w 15), 16 positions, every hand-off taken, the first-round
// and the last three lengths held at the same rows while the ten positions between them were cut in two: 0.8653 -> 0.8792 ms per
// step for 10 more segment sets = 1.39 us per set, against 2.0 us per row of a set (0.743 ms SAD stage / 372 row times); cut in
// three, 8 rows each, 2.0 us. 640x480 nd 64 w 21 x64 the same way: 0.93 us per set against 0.72 us per row, 9 % of those
// hand-offs missed and primed (profiles/r07_sad_segment_plan.txt, table 1).
//
// One rule for the lengths: they rise over the first round of the chip (positions 0 .. D-2, which start together: 10 % of a
// regular segment per position, kFirstRoundStep, so that their sets finish in dispatch order), reach the regular length at
// position D-1, and from there FALL LINEARLY to 1 / (n - D + 1) of it at the last position. Every round of the chip is then
// shorter than the one before, the sets keep finishing in dispatch order, and the last, partly empty round lasts as long as the
// shortest segments instead of a quarter of a regular one. Rows that the rounding leaves over go one each to the positions from
// D-1 on, so the rise stays a rise and the last position stays the shortest. A flat middle with a taper over the last 3, 6, 9
// or 12 positions, a geometric taper and shorter take-over positions behind a regular first round all measured slower or equal
// (same file, tables 2 and 3).
//
// The count: as sad_fast_plan's model with the hand-off's price in place of the priming rows, n = sqrt(c' * slots * rows /
// (per_seg * kHandoffRows)) -- but the tail this shape leaves is shorter than the 3/4, 1/2, 1/4 taper's that c = 0.196 was fitted
// on, so c' = kSegCLinked = 0.12, fitted on the sweeps of that file: KITTI x64 flat within 0.002 ms from 12 to 16 (rule: 13),
// 640x480 nd 64 w 21 x64 from 14 to 22 (22), KITTI nd 64 x64 from 11 to 15 (14); 8 KITTI pairs and 16 pairs 640x480, where
// sad_fast_plan's fill rule already asks for more, best at 40 and 48 (35, 45). Past the flat part the time RISES with the count
// (KITTI x64: 0.858 at 16, 0.867 at 20, 0.885 at 32): short segments pay more than 0.7 of a row per hand-off.
// Never fewer segments than sad_fast_plan's, and no more than fit kHandoffMaxBytes of slots.
constexpr double kHandoffRows = 0.7, kSegCLinked = 0.12;
static int fast_linked_plan(const Geom& g, int rows, long per_seg, int slots, int nseg, int maxseg, int* len) {
  if (nseg < 3 || (g.nd != 32 && g.nd != 64 && g.nd != 128)) return 0;
  unsigned char at[64];
  const int D = fast_segment_order(nseg, per_seg, slots, g.nd, at);
  if (D >= nseg) return 0;
  int n = (int)(std::sqrt(kSegCLinked * slots * rows / ((double)per_seg * kHandoffRows)) + 0.5);
  n = std::max(nseg, std::min(n, std::min(maxseg, 64)));
  size_t fb;
  while (n > nseg && fast_handoff_size(n - D, per_seg, g.nd, &fb) > kHandoffMaxBytes) n--;
  if (fast_handoff_size(n - D, per_seg, g.nd, &fb) > kHandoffMaxBytes) return 0;
  const int fr = D - 1;   // positions of the first round
  const double step = fr > 1 ? std::min(kFirstRoundStep, kFirstRoundSpan / (fr - 1)) : 0.0;
  double wgt[64], sum = 0;
  for (int p = 0; p < n; p++) {
    wgt[p] = p < fr ? 1.0 - step * (fr - 1 - p) : (double)(n - p) / (n - fr);
    sum += wgt[p];
  }
  const double unit = rows / sum;
  int left = rows;
  for (int p = 0; p < n; p++) {
    len[p] = (int)(wgt[p] * unit);
    left -= len[p];
  }
  for (int p = fr; p < n && left > 0; p++, left--) len[p]++;
  for (int p = fr - 1; p >= 0 && left > 0; p--, left--) len[p]++;
  return n;
}

// The interior launch of a call with pl->fast: strips, row segments, split, then -- through the window and layout dispatch, which
// knows the per-instantiation constants -- the border jobs, grid, LDS and the kernel's name.
void sad_fast_plan(BmPlan* pl) {
  const Geom& g = pl->g;
  FastPlan& a = pl->f;
  const int xhi = std::min(g.W - g.lofs - 1, g.W - g.rofs - g.nd);
  a.xc0 = g.w2; a.xc1 = xhi - g.w2 + 1;
  const int pw = g.wsz % 3 == 0 ? 3 : 1;
  const int nv = 64 - (g.wsz - pw);
  // windows that are multiples of 3: triples of column-stride-3 strips (3 * nv3 columns each) as far as they pay, plain
  // strips for the rest (SBM_FAST_CS3=0: plain strips only)
  const int cs3_env = env_switch("SBM_FAST_CS3", 1);   // read per call (the GPU tests flip it)
  const int ncols = a.xc1 - a.xc0;
  const int nv3 = 64 - (g.wsz / 3 - 1);
  int triples = 0;
  if (pw == 3 && cs3_env) {
    triples = ncols / (3 * nv3);
    if (ncols - triples * 3 * nv3 > 2 * nv) triples++;   // a remainder worth three plain strips is one more triple
  }
  a.strips3 = 3 * triples;
  const int rem = std::max(0, ncols - triples * 3 * nv3);
  const int strips = a.strips3 + (rem + nv - 1) / nv;
  const int rows = g.row1 - g.row0;
  // Row segments. Every segment pays w - 1 priming rows (~0.2 of a full row each: mqsad only); few long segments keep that low,
  // many short ones keep the tail of the launch short (the last, partly empty round of workgroups). With R rounds of the chip
  // the two costs are ~ prime * nseg / rows and ~ c / R, R = strips * pairs * nseg / slots, so the optimum is
  //   nseg = sqrt(c * slots * rows / (strips * pairs * prime)),   slots = workgroups the chip holds at once for the layout
  // (4 096 / 3 072 / 1 536 at up to 64 / 128 / 256 disparities), c = 0.196 fitted on the forced-count sweeps of round 5
  // (profiles/r05_small_launch_segments.txt, last table: KITTI x64 best at 8 = the formula's 8.0; 640x480 nd 64 w 21 x64 best at
  // 10-14, formula 12, round 4's rule 6: 0.476 -> 0.469 ms; 1080p nd 256 x64 best 6-8, formula 6.6, round 4's 4: 8.28 -> 8.19;
  // 2160p x32 best 8-12, formula 9, round 4's 3: 17.64 -> 16.97; 1080p x16 and 2160p x4 unchanged at 13 and 25). Round 4's rule
  // (a workgroup target of 24 000 / 5 600 with segments of at least three window heights) was tuned at 64 / 16 / 4 pairs only.
  // Where segments take their sums over (fast_segment_order) this count is only the start: fast_linked_plan below re-counts with
  // the price of a hand-off in place of the priming rows and gives the lengths another shape.
  // (one round of the chip for the cooperating 128-disparity wavefronts: 12 wavefronts per CU in workgroups of 2 / 3 / 4)
  const int round1 = g.nd <= 256 ? 1536 : (g.nd <= 384 ? 1024 : 768);
  constexpr double kSegC = 0.196;   // c of the model above
  const int slots_i = g.nd <= 64 ? 4096 : (g.nd <= 128 ? 3072 : round1);
  int nseg = 1;
  {
    const double prime = 0.2 * (g.wsz - 1);
    const double slots = slots_i;
    nseg = (int)(std::sqrt(kSegC * slots * rows / ((double)strips * g.n * prime)) + 0.5);
    nseg = std::max(1, std::min(nseg, std::max(1, rows / g.wsz)));   // (at least one window height per segment here; see below)
  }
  // Launches that do not fill the chip (round 5, profiles/r05_small_launch_segments.txt): a wavefront's row segment is a serial
  // chain, and w - 1 priming rows at a third of a row's cost are cheaper than idle SIMDs -- segments go down to 8 rows (up to
  // 64 of them) until the launch has ~5 000 workgroups. Launches that cannot even reach ~1 800 wavefronts that way (one or two
  // pairs) split the disparities over more wavefronts per workgroup instead (launch_nd: `split`) and take as many segments
  // as keep them under 1 024 workgroups. One 640x480 nd 64 w 21 pair: SAD stage 0.054 -> 0.049 ms, one KITTI pair 0.052 ->
  // 0.036, 8 KITTI pairs 0.209 -> 0.14, 16 pairs 640x480 0.203 -> 0.12, 4 pairs 1080p nd 256 0.64 -> 0.57.
  constexpr int kSmallRows = 8;   // shortest row segment of a launch that does not fill the chip
  constexpr long kFill = 5000;     // workgroups such a launch is cut into
  const int maxseg = std::max(nseg, std::min(64, rows / kSmallRows));
  const long per_seg = (long)strips * g.n;
  if (per_seg * maxseg * (g.nd > 128 ? (g.nd + 127) / 128 : 1) < 1800) {
    nseg = std::max(nseg, (int)std::min<long>(maxseg, 1023 / per_seg));
  } else {
    const int nseg1 = nseg;
    while (per_seg * nseg < kFill && nseg < maxseg) nseg++;
    // (two cooperating 128-disparity wavefronts: 1 536 workgroups are one round of the chip; a launch that ends between 1 and
    // 1.5 rounds pays a second, mostly empty round -- one 1080p nd 256 pair: 64 segments 0.204 ms, 36..48 segments 0.189..0.196)
    if (g.nd > 128 && per_seg * nseg > round1 && 2 * per_seg * nseg < 3 * round1) nseg = std::max(nseg1, (int)((long)round1 * 1450 / 1536 / per_seg));
  }
  // taper: the last third of the rows is cut into segments of 2/3, 1/2, 1/3 ... of the regular length
  nseg = std::min(nseg, 64);
  int len[64];
  const int linked = fast_linked_plan(g, rows, per_seg, slots_i, nseg, maxseg, len);   // (0: not linked -- the lengths below)
  int ns = 0;
  a.segrow[0] = g.row0;
  if (nseg < 3) {
    const int seg = (rows + nseg - 1) / nseg;
    for (int y = g.row0; y < g.row1; y += seg) a.segrow[++ns] = std::min(y + seg, g.row1);
  } else {
    // The weights go by DISPATCH POSITION (fast_segment_order: which segment a position holds): 1, ..., 1, 3/4, 1/2, 1/4 --
    // fewer rows to prime than nseg equal ones, and the last workgroups of the launch are short. Where the order is not the
    // identity (segments take their sums over), the positions of the first round of the chip -- every one of them starts when the
    // launch does -- also get 10 % fewer rows per position they lie in front of that round's last one (kFirstRoundStep): their sets then finish
    // one after the other, in dispatch order, which is what the order's distance rule counts on.
    unsigned char at[64];
    const int stride = fast_segment_order(nseg, per_seg, slots_i, g.nd, at);
    const int first_round = stride - 1;
    if (linked) {
      nseg = linked;
    } else {
      // (many small sets in the first round: the steps shrink so that its first set keeps 1 - kFirstRoundSpan of a regular one)
      const double step = first_round > 1 ? std::min(kFirstRoundStep, kFirstRoundSpan / (first_round - 1)) : 0.0;
      double wgt[64], sum = 0;
      for (int p = 0; p < nseg; p++) {
        wgt[p] = p < nseg - 3 ? 1.0 : (p == nseg - 3 ? 0.75 : (p == nseg - 2 ? 0.5 : 0.25));
        if (stride < nseg && p < first_round) wgt[p] = std::min(wgt[p], 1.0 - step * (first_round - 1 - p));
        sum += wgt[p];
      }
      const double unit = rows / sum;
      double acc = 0;
      int y0 = 0;
      for (int p = 0; p < nseg; p++) {
        acc += wgt[p] * unit;
        const int y1 = p == nseg - 1 ? rows : std::min(rows, (int)(acc + 0.5));
        len[p] = y1 - y0;
        y0 = y1;
      }
    }
    // positions that got no row drop out; the order is the one of the segments that remain
    int np = 0;
    for (int p = 0; p < nseg; p++)
      if (len[p] > 0) len[np++] = len[p];
    fast_segment_order(np, per_seg, slots_i, g.nd, at);
    int seglen[64];
    for (int p = 0; p < np; p++) seglen[at[p]] = len[p];
    for (int k = 0; k < np; k++) a.segrow[k + 1] = a.segrow[k] + seglen[k];
    ns = np;
  }
  nseg = ns;
  a.strips = strips; a.nseg = nseg;
  {
    const long maxs = (long)g.wsz * g.wsz * 2 * g.cap;
    a.uniq_plain = 8 * ((maxs * g.uniq / 100 + 1) << g.pfshift) <= 65535;   // (8 registers per accumulator)
  }
  a.split = (long)strips * nseg * g.n < 1024;
  sad_fast_dispatch(*pl, nullptr, nullptr);   // no arguments: the dispatch fills the plan
}

// The folded leftover strip (sbm_sad_fast_fold.h): the columns R of the launch's last strip if that strip runs folded, else 0.
// It does when the strip is a plain one with R <= FoldLds::NV = 22 columns, the window is 15, the count exactly 128 and the layout
// the lone wavefront -- KITTI: 1 101 interior columns = 18 stride-3 strips + 21. SBM_FAST_FOLD=0 (read per call: the GPU tests
// flip it) keeps the plain strip.
int sad_fast_fold_cols(const BmPlan& pl) {
  const FastPlan& f = pl.f;
  if (!pl.fast || env_switch("SBM_FAST_FOLD", 1) == 0) return 0;
  if (f.NDW != FoldLds::NDW || f.NWAVES != 1 || !f.exact || f.NTERM * f.PW != FoldLds::NTERM * FoldLds::PW || !f.dual) return 0;
  if (f.strips <= f.strips3) return 0;   // (no plain strip)
  const int nv3 = 64 - (f.NTERM - 1), nv1 = 64 - f.PW * (f.NTERM - 1);
  const int cols = (f.xc1 - f.xc0) - ((f.strips3 / 3) * 3 * nv3 + (f.strips - 1 - f.strips3) * nv1);
  return cols >= 1 && cols <= FoldLds::NV ? cols : 0;
}

// Which segments take their sums over in this call (bit k: segment k from k - 1) and the dispatch order that goes with it: none
// with cooperating wavefronts, a masked count or SBM_FAST_HANDOFF=0, every later segment where the segments are launches of their own, else
// the segments behind the first D positions of fast_segment_order().
static unsigned long long fast_handoff_links(const BmPlan& pl, unsigned char* at) {
  const FastPlan& f = pl.f;
  const int mode = fast_handoff_mode();
  const int stride = fast_segment_order(f.nseg, (long)f.strips * pl.g.n, fast_slots(pl.g.nd), pl.g.nd, at);
  if (mode == 0 || f.NWAVES != 1 || !f.exact || f.nseg < 2) return 0;   // (FastHandoff<>::ON)
  unsigned long long links = 0;
  for (int p = mode == 2 ? 1 : stride; p < f.nseg; p++) links |= 1ull << at[p];
  return links;
}

// sad_fast_handoff_bytes: fast_handoff_size() of the call's linked segments. 0: this call hands nothing over (also where the slots
// would take more than kHandoffMaxBytes: it primes instead).
size_t sad_fast_handoff_bytes(const BmPlan& pl, size_t* flag_bytes) {
  unsigned char at[64];
  *flag_bytes = 0;
  if (!pl.fast) return 0;
  const unsigned long long links = fast_handoff_links(pl, at);
  if (!links) return 0;
  size_t fb = 0;
  const size_t bytes = fast_handoff_size(__builtin_popcountll(links), (long)pl.g.n * pl.f.strips, pl.f.NDW, &fb);
  if (bytes > kHandoffMaxBytes) return 0;
  *flag_bytes = fb;
  return bytes;
}

// The arguments of the planned launch. handoff: sad_fast_handoff_bytes() of scratch whose ready and taken words no earlier
// launch has written `epoch` to (null: nothing is handed over); *links: how many (segment, pair, strip) may take their sums over.
hipError_t launch_sad_fast(const uint8_t* pf_l, const uint8_t* pf_r, int16_t* disp, int32_t* cost, BmPlan& pl, void* handoff,
                           unsigned epoch, long* links, hipStream_t s) {
  const Geom& g = pl.g;
  const FastPlan& f = pl.f;
  FastArgs a;
  a.pf_l = pf_l; a.pf_r = pf_r; a.disp = disp; a.cost = g.want_cost ? reinterpret_cast<uint16_t*>(cost) : nullptr;
  a.W = g.W; a.H = g.H; a.pitch = g.pitch; a.padl = g.padl; a.plane = g.plane;
  a.nd = g.nd; a.mindisp = g.mindisp; a.lofs = g.lofs; a.rofs = g.rofs; a.tex = g.tex << g.pfshift; a.uniq = g.uniq;
  a.filtered = g.filtered; a.capb = (g.cap << g.pfshift) + kPfBias; a.pfshift = g.pfshift;
  a.row0 = g.row0; a.row1 = g.row1;
  static_assert(sizeof(a.segrow) == sizeof(f.segrow), "");
  memcpy(a.segrow, f.segrow, sizeof(a.segrow));
  a.strips = f.strips; a.nseg = f.nseg; a.npairs = g.n; a.strips3 = f.strips3; a.uniq_plain = f.uniq_plain;
  a.xc0 = f.xc0; a.xc1 = f.xc1;
  a.fold = sad_fast_fold_cols(pl) > 0;
  a.nbr_tree = env_switch("SBM_FAST_NBR", 1) == 0;   // (read per call, as SBM_FAST_FOLD: the GPU tests flip it)
  a.bord = f.bord; a.bnw = f.bnw; a.bseg = f.bseg; a.nbseg = f.nbseg;
  a.ho_link = fast_handoff_links(pl, a.segat);   // (fills the order)
  if (!handoff) a.ho_link = 0;
  a.ho = static_cast<u32*>(handoff); a.ho_epoch = epoch;
  a.segbase = 0; a.grid = f.grid;
  const long per_seg = (long)f.strips * g.n;
  *links = (long)__builtin_popcountll(a.ho_link) * per_seg;
  if (fast_handoff_mode() != 2 || !a.ho_link) return sad_fast_dispatch(pl, &a, s);
  // the segments as launches of their own, top to bottom (the order is the identity); the border jobs ride in the first
  for (int k = 0; k < f.nseg; k++) {
    a.segbase = k;
    a.grid = (int)per_seg + (k == 0 ? f.bord * f.nbseg : 0);
    if (k == 1) a.bord = 0;
    const hipError_t e = sad_fast_dispatch(pl, &a, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace sbm
