// Visual-word dictionary and loop-closure likelihood of the reference's loop-closure thread: addWordIds -> VWDictionary::addNewWords
// (src/slam/src/core/Mapper.cpp:413-484, VWDictionary.cpp:40-115), detectLoopClosure -> computeLikelihood (Mapper.cpp:536-677) and
// SensorData::limitKeypoints (SensorData.cpp:109-133). include/sbm.h ("visual-word dictionary") states the semantics, DESIGN.md
// section 16 the readings. The search is exhaustive where the reference's FLANN kd-trees (32 checks) are approximate.
//
//   search   one wavefront per (64-query tile, dictionary slice): each lane keeps its query row in 8 VGPRs; the slice's words (and
//            for L2 their squared norms) pass through LDS 64 at a time and are read as broadcasts; per word 8 accumulating
//            v_sad_u8 (L1) or 8 accumulating v_dot4_u32_u8 and |a|^2 + |b|^2 - 2 a.b (L2), then the 2-NN update. Partial records
//            (i0, d0, i1, d1) per slice go to scratch.
//   decide   one lane per query: merges the slices in dictionary order (a later word replaces a neighbour only when strictly
//            nearer, so neighbours are ordered by (distance, index)), writes the record and the uniqueness flag.
//   append   one workgroup: counts the unique rows; when they fit, a ballot + prefix scan in row order gives each its slot
//            size + rank, the rows (and norms) are copied there, every row's word id is written, and the new size. Searches read
//            rows < size and the append writes rows >= size.
// The host keeps, per word, its references (node -> count) and, per node, its word ids and keypoint count, from the ids that come
// back. Nothing here contracts a multiply-add (the pragmas below and -ffp-contract=off).
#include <math.h>

#include <algorithm>
#include <climits>
#include <map>
#include <new>
#include <numeric>
#include <vector>

#include "sbm_handle.h"

namespace sbm {
namespace {

struct VwdNode {
  std::vector<int> words;   // word id of every row added for this node, in row order
  long long ni;             // keypoints of the node, the ones cut by the limit included
};

}  // namespace
}  // namespace sbm

struct sbm_vwd {
  sbm_handle* h;
  sbm_vwd_params p;
  size_t capacity;                         // words the caller asked for
  size_t size;                             // the device's size, as of the last synchronous read
  sbm::DevBuf rows, norm, ctr;             // 32 bytes and one squared norm per word; VwdCounters
  std::vector<std::map<int, int>> refs;    // per word: node -> count
  std::map<int, sbm::VwdNode> nodes;
  template <class F> void each(F f) { f(rows); f(norm); f(ctr); }
};

namespace sbm {
namespace {

constexpr int kTile = 64;              // queries per wavefront (= workgroup)
constexpr int kStage = 64;             // words per LDS stage
constexpr int kTargetWaves = 4096;     // slices are added until a launch has about this many wavefronts (16 per CU)
constexpr int kMaxSlice = 65535;       // gridDim.y
constexpr int kMaxQueries = 65535;
constexpr size_t kMaxCapacity = (size_t)1 << 26;   // 2 GiB of rows; indices and byte offsets stay far inside their types

struct VwdCounters {
  unsigned long long overflow;   // calls refused because their new words did not fit
  unsigned size;                 // words in the store
  unsigned added;                // new words of the last call
};

__device__ __forceinline__ unsigned dot4(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_udot4(a, b, c, false); }

template <int kMetric> __device__ __forceinline__ unsigned row_term(const uint4& a, const uint4& b, unsigned acc) {
  if (kMetric == SBM_VWD_L1) {
    acc = __builtin_amdgcn_sad_u8(a.x, b.x, acc);
    acc = __builtin_amdgcn_sad_u8(a.y, b.y, acc);
    acc = __builtin_amdgcn_sad_u8(a.z, b.z, acc);
    return __builtin_amdgcn_sad_u8(a.w, b.w, acc);
  }
  return dot4(a.w, b.w, dot4(a.z, b.z, dot4(a.y, b.y, dot4(a.x, b.x, acc))));
}

// (i0, d0, i1, d1) <- the word (idx, d), which comes after every word seen so far: it takes a place only when strictly nearer
__device__ __forceinline__ void knn_push(int4& r, int idx, int d) {
  if (d < r.y) {
    r.z = r.x;
    r.w = r.y;
    r.x = idx;
    r.y = d;
  } else if (d < r.w) {
    r.z = idx;
    r.w = d;
  }
}

template <int kMetric>
__global__ void __launch_bounds__(64) vwd_search_kernel(const uint8_t* __restrict__ desc, int n, const uint8_t* __restrict__ rows,
                                                        const unsigned* __restrict__ norm, const VwdCounters* __restrict__ ctr,
                                                        int slice_rows, int4* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint4 s_row[kStage][2];
  __shared__ unsigned s_norm[kStage];
  const int lane = threadIdx.x, slice = blockIdx.y;
  const int q = blockIdx.x * kTile + lane;
  const int N = (int)ctr->size;
  const long long r0l = (long long)slice * slice_rows;
  if (r0l >= N) return;   // uniform over the workgroup; the decide kernel reads no such slice
  const int r0 = (int)r0l, r1 = (int)min((long long)N, r0l + slice_rows);

  uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
  if (q < n) {
    const uint4* qa = (const uint4*)(desc + (size_t)q * 32);
    a0 = qa[0];
    a1 = qa[1];
  }
  unsigned na = 0;
  if (kMetric == SBM_VWD_L2) na = row_term<kMetric>(a1, a1, row_term<kMetric>(a0, a0, 0u));
  int4 rec = make_int4(-1, SBM_VWD_NONE, -1, SBM_VWD_NONE);
  const uint4* wrow = (const uint4*)rows;
  for (int c0 = r0; c0 < r1; c0 += kStage) {
    const int nr = min(kStage, r1 - c0);
    __syncthreads();   // the previous stage has been read
    if (lane < nr) {
      s_row[lane][0] = wrow[2 * (size_t)(c0 + lane)];
      s_row[lane][1] = wrow[2 * (size_t)(c0 + lane) + 1];
      if (kMetric == SBM_VWD_L2) s_norm[lane] = norm[c0 + lane];
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < nr; k++) {
      const uint4 b0 = s_row[k][0], b1 = s_row[k][1];
      const unsigned t = row_term<kMetric>(a1, b1, row_term<kMetric>(a0, b0, 0u));
      const int d = kMetric == SBM_VWD_L1 ? (int)t : (int)(na + s_norm[k] - 2u * t);
      knn_push(rec, c0 + k, d);
    }
  }
  if (q < n) part[(size_t)slice * n + q] = rec;
}

// Merges the slices of every query in dictionary order and takes the uniqueness decision of addNewWords.
__global__ void __launch_bounds__(256) vwd_decide_kernel(int n, const VwdCounters* __restrict__ ctr, int slice_rows, int nslice,
                                                         float nndr, const int4* __restrict__ part, int4* __restrict__ knn,
                                                         uint8_t* __restrict__ unique) {
#pragma clang fp contract(off)
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const int N = (int)ctr->size;
  const int ns = (int)min((long long)nslice, ((long long)N + slice_rows - 1) / slice_rows);
  int4 rec = make_int4(-1, SBM_VWD_NONE, -1, SBM_VWD_NONE);
  for (int s = 0; s < ns; s++) {
    const int4 r = part[(size_t)s * n + q];
    if (r.x >= 0) knn_push(rec, r.x, r.y);
    if (r.z >= 0) knn_push(rec, r.z, r.w);
  }
  knn[q] = rec;
  if (unique) {
    const float lim = nndr * (float)rec.w;   // one multiply, one compare
    unique[q] = (rec.z < 0 || (float)rec.y > lim) ? 1 : 0;
  }
}

template <int kMetric>
__global__ void __launch_bounds__(256) vwd_append_kernel(const uint8_t* __restrict__ desc, int n, const int4* __restrict__ knn,
                                                         const uint8_t* __restrict__ unique, unsigned capacity,
                                                         uint8_t* __restrict__ rows, unsigned* __restrict__ norm,
                                                         VwdCounters* __restrict__ ctr, int* __restrict__ ids) {
  __shared__ int s_wave[4];
  __shared__ int s_total;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned size = ctr->size;
  if (tid == 0) s_total = 0;
  __syncthreads();
  int mine = 0;
  for (int q = tid; q < n; q += 256) mine += unique[q];
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  if (lane == 0) atomicAdd(&s_total, mine);
  __syncthreads();
  const int total = s_total;
  if ((unsigned long long)size + (unsigned)total > capacity) {   // nothing is added: no row, no id, the size stays
    for (int q = tid; q < n; q += 256) ids[q] = -1;
    if (tid == 0) {
      ctr->overflow += 1;
      ctr->added = 0;
    }
    return;
  }
  int placed = 0;
  for (int base = 0; base < n; base += 256) {
    const int q = base + tid;
    const bool u = q < n && unique[q] != 0;
    const unsigned long long m = __ballot(u);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();   // the previous round's counts have been read
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int off = placed;
    for (int w = 0; w < wv; w++) off += s_wave[w];
    placed += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (u) {
      const size_t slot = (size_t)size + (unsigned)(off + below);   // < capacity: off + below < total
      const uint4* src = (const uint4*)(desc + (size_t)q * 32);
      const uint4 a0 = src[0], a1 = src[1];
      uint4* dst = (uint4*)(rows + slot * 32);
      dst[0] = a0;
      dst[1] = a1;
      if (kMetric == SBM_VWD_L2) norm[slot] = row_term<kMetric>(a1, a1, row_term<kMetric>(a0, a0, 0u));
      ids[q] = (int)slot;
    } else if (q < n) {
      ids[q] = knn[q].x;
    }
  }
  if (tid == 0) {
    ctr->size = size + (unsigned)total;
    ctr->added = (unsigned)total;
  }
}

}  // namespace

enum VwdStage { kVwSearch, kVwAppend, kVwTotal, kVwStageCount };
enum VwdMark { kVwBegin, kVwMid, kVwEnd, kVwMarkCount };
static const char* const kVwdNames[] = {"vwd_search", "vwd_append", "vwd_total"};
StageTable vwd_stages() { return stage_table<kVwStageCount, kVwMarkCount>(kVwdNames); }

}  // namespace sbm

using namespace sbm;

// The launch plan of a search of n queries against N words: slice s covers words [s * slice_rows, (s + 1) * slice_rows).
static void vwd_plan(int n, size_t N, int want, int* nslice, int* slice_rows) {
  const long long stages = std::max<long long>(1, ((long long)N + kStage - 1) / kStage);
  const int qtiles = std::max(1, (n + kTile - 1) / kTile);
  long long ns = want > 0 ? want : (kTargetWaves + qtiles - 1) / qtiles;
  ns = std::max<long long>(1, std::min<long long>({ns, stages, (long long)kMaxSlice}));
  const long long per = (stages + ns - 1) / ns * kStage;
  *slice_rows = (int)per;
  *nslice = (int)((stages * kStage + per - 1) / per);
}

static int vwd_read_counters(sbm_vwd* v, VwdCounters* c) {
  sbm_handle* h = v->h;
  HIPCHK(h, hipMemcpyAsync(c, v->ctr.p, sizeof(*c), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  v->size = c->size;
  return SBM_OK;
}

static int vwd_clear(sbm_vwd* v) {
  HIPCHK(v->h, hipMemsetAsync(v->ctr.p, 0, sizeof(VwdCounters), v->h->stream));
  v->size = 0;
  v->refs.clear();
  v->nodes.clear();
  return SBM_OK;
}

// Search + decide (+ append when d_ids is given) of n > 0 queries on the handle's stream. Scratch: partial records of every slice,
// then the merged records and the flags.
static int vwd_run(sbm_vwd* v, const uint8_t* d_desc, int n, int4* d_knn_out, int* d_ids) {
  sbm_handle* h = v->h;
  StageClock& clk = h->vwd.clock;
  HIPCHK(h, clk.start(vwd_stages(), h->profiling != 0));
  int nslice, slice_rows;
  vwd_plan(n, v->size, v->p.slices, &nslice, &slice_rows);
  int4 *part, *knn;
  uint8_t* unique;
  HIPCHK(h, carve(h->vwd.scratch, h->stream, [&](Carve& c) { part = c.take<int4>((size_t)nslice * n); knn = c.take<int4>(n); unique = c.take<uint8_t>(n); }));
  if (d_knn_out) knn = d_knn_out;
  if (!d_ids) unique = nullptr;
  const VwdCounters* ctr = v->ctr.as<VwdCounters>();
  const bool l2 = v->p.metric == SBM_VWD_L2;
  const dim3 gs((n + kTile - 1) / kTile, nslice);
  HIPCHK(h, clk.mark(kVwBegin, h->stream));
  if (v->size > 0) {   // an empty dictionary has no slice to search
    if (l2)
      hipLaunchKernelGGL(vwd_search_kernel<SBM_VWD_L2>, gs, dim3(64), 0, h->stream, d_desc, n, v->rows.as<uint8_t>(),
                         v->norm.as<unsigned>(), ctr, slice_rows, part);
    else
      hipLaunchKernelGGL(vwd_search_kernel<SBM_VWD_L1>, gs, dim3(64), 0, h->stream, d_desc, n, v->rows.as<uint8_t>(),
                         v->norm.as<unsigned>(), ctr, slice_rows, part);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, clk.mark(kVwMid, h->stream));
  hipLaunchKernelGGL(vwd_decide_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, ctr, slice_rows, nslice, v->p.nndr,
                     (const int4*)part, knn, unique);
  HIPCHK(h, hipGetLastError());
  if (d_ids) {
    if (l2)
      hipLaunchKernelGGL(vwd_append_kernel<SBM_VWD_L2>, dim3(1), dim3(256), 0, h->stream, d_desc, n, (const int4*)knn,
                         (const uint8_t*)unique, (unsigned)v->capacity, v->rows.as<uint8_t>(), v->norm.as<unsigned>(),
                         v->ctr.as<VwdCounters>(), d_ids);
    else
      hipLaunchKernelGGL(vwd_append_kernel<SBM_VWD_L1>, dim3(1), dim3(256), 0, h->stream, d_desc, n, (const int4*)knn,
                         (const uint8_t*)unique, (unsigned)v->capacity, v->rows.as<uint8_t>(), v->norm.as<unsigned>(),
                         v->ctr.as<VwdCounters>(), d_ids);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, clk.mark(kVwEnd, h->stream));
  HIPCHK(h, clk.add(kVwSearch, kVwBegin, kVwMid));
  HIPCHK(h, clk.add(kVwAppend, kVwMid, kVwEnd));
  if (clk.on) clk.ms[kVwTotal] = clk.ms[kVwSearch] + clk.ms[kVwAppend];
  return SBM_OK;
}

// addNewWords' bookkeeping from the ids of one call: a new word (ids count on from old_size in row order) gets the reference
// (node, 1), any other row is addRef(node) on its word; the node keeps its ids and its keypoint count.
static void vwd_book(sbm_vwd* v, size_t old_size, const int* ids, int n, int node_id, int n_keypoints_total) {
  VwdNode& node = v->nodes[node_id];
  node.ni += n_keypoints_total;
  for (int i = 0; i < n; i++) {
    const int id = ids[i];
    if ((size_t)id >= old_size && (size_t)id == v->refs.size()) v->refs.emplace_back();
    v->refs[(size_t)id][node_id] += 1;
    node.words.push_back(id);
  }
}

static int vwd_add(sbm_vwd* v, const uint8_t* d_desc, int n, int node_id, int n_keypoints_total, int* word_ids) {
  sbm_handle* h = v->h;
  std::vector<int> ids;
  try {
    ids.resize((size_t)std::max(n, 1));
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  if (n == 0) {
    try {
      vwd_book(v, v->size, ids.data(), 0, node_id, n_keypoints_total);
    } catch (const std::bad_alloc&) {
      return SBM_ERR_NOMEM;
    }
    return SBM_OK;
  }
  HIPCHK(h, h->vwd.ids.grow((size_t)n * sizeof(int), h->stream));
  const size_t old_size = v->size;
  int st = vwd_run(v, d_desc, n, nullptr, h->vwd.ids.as<int>());
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpyAsync(ids.data(), h->vwd.ids.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  VwdCounters c;
  st = vwd_read_counters(v, &c);
  if (st != SBM_OK) return st;
  if (c.size == old_size && ids[0] < 0) return SBM_ERR_VWD_FULL;   // refused: every id is -1
  try {
    vwd_book(v, old_size, ids.data(), n, node_id, n_keypoints_total);
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  if (word_ids) memcpy(word_ids, ids.data(), (size_t)n * sizeof(int));
  return SBM_OK;
}

static int vwd_check_add(const sbm_vwd* v, const void* desc, int n, int node_id, int n_keypoints_total) {
  if (!v || (n > 0 && !desc)) return SBM_ERR_NULL;
  if (n < 0 || n > kMaxQueries || n_keypoints_total < n) return SBM_ERR_SIZE;
  if (node_id < 1) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

extern "C" {

void sbm_vwd_params_default(sbm_vwd_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->metric = SBM_VWD_L1;
  p->nndr = 0.8f;
  p->slices = 0;
}

int sbm_vwd_params_validate(const sbm_vwd_params* p) {
  if (!p) return SBM_ERR_NULL;
  if (p->metric != SBM_VWD_L1 && p->metric != SBM_VWD_L2) return SBM_ERR_UNSUPPORTED;
  if (!(p->nndr > 0.f && p->nndr <= 1.f)) return SBM_ERR_UNSUPPORTED;   // NaN fails both
  if (p->slices < 0 || p->slices > kMaxSlice) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

int sbm_vwd_create(sbm_handle* h, size_t capacity, const sbm_vwd_params* p, sbm_vwd** out) {
  if (!h || !p || !out) return SBM_ERR_NULL;
  *out = nullptr;
  int st = sbm_vwd_params_validate(p);
  if (st != SBM_OK) return st;
  if (capacity < 1) return SBM_ERR_SIZE;
  if (capacity > kMaxCapacity) return SBM_ERR_UNSUPPORTED;
  sbm_vwd* v = new (std::nothrow) sbm_vwd();
  if (!v) return SBM_ERR_NOMEM;
  v->h = h;
  v->p = *p;
  v->capacity = capacity;
  DeviceScope dscope(h->device);
  hipError_t e = dscope.enter();
  if (e == hipSuccess) e = v->rows.grow(capacity * 32, h->stream);
  if (e == hipSuccess) e = v->norm.grow(capacity * sizeof(unsigned), h->stream);
  if (e == hipSuccess) e = v->ctr.grow(sizeof(VwdCounters), h->stream);
  st = SBM_OK;
  if (e != hipSuccess) {
    h->last_hip = (int)e;
    st = e == hipErrorOutOfMemory ? SBM_ERR_NOMEM : SBM_ERR_HIP;
  }
  if (st == SBM_OK) st = vwd_clear(v);
  if (st != SBM_OK) {
    release_all(*v);
    delete v;
    return st;
  }
  *out = v;
  return SBM_OK;
}

void sbm_vwd_destroy(sbm_vwd* v) {
  if (!v) return;
  DeviceScope dscope(v->h->device);
  dscope.enter();
  hipStreamSynchronize(v->h->stream);
  release_all(*v);
  delete v;
}

int sbm_vwd_reset(sbm_vwd* v) {
  if (!v) return SBM_ERR_NULL;
  DeviceScope dscope(v->h->device);
  HIPCHK(v->h, dscope.enter());
  return vwd_clear(v);
}

int sbm_vwd_size(sbm_vwd* v, size_t* size) {
  if (!v || !size) return SBM_ERR_NULL;
  DeviceScope dscope(v->h->device);
  HIPCHK(v->h, dscope.enter());
  VwdCounters c;
  const int st = vwd_read_counters(v, &c);
  if (st == SBM_OK) *size = c.size;
  return st;
}

int sbm_vwd_overflow(sbm_vwd* v, uint64_t* overflow) {
  if (!v || !overflow) return SBM_ERR_NULL;
  DeviceScope dscope(v->h->device);
  HIPCHK(v->h, dscope.enter());
  VwdCounters c;
  const int st = vwd_read_counters(v, &c);
  if (st == SBM_OK) *overflow = c.overflow;
  return st;
}

int sbm_vwd_add_words_device(sbm_vwd* v, const void* d_desc, int n, int node_id, int n_keypoints_total, int* word_ids) {
  const int st = vwd_check_add(v, d_desc, n, node_id, n_keypoints_total);
  if (st != SBM_OK) return st;
  if ((uintptr_t)d_desc & 15) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(v->h->device);
  HIPCHK(v->h, dscope.enter());
  return vwd_add(v, (const uint8_t*)d_desc, n, node_id, n_keypoints_total, word_ids);
}

int sbm_vwd_add_words(sbm_vwd* v, const uint8_t* desc, size_t stride, int n, int node_id, int n_keypoints_total, int* word_ids) {
  const int st = vwd_check_add(v, desc, n, node_id, n_keypoints_total);
  if (st != SBM_OK) return st;
  if (n > 0 && stride < 32) return SBM_ERR_SIZE;
  sbm_handle* h = v->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  if (n > 0) {
    HIPCHK(h, h->vwd.io.grow((size_t)n * 32, h->stream));
    HIPCHK(h, hipMemcpy2DAsync(h->vwd.io.p, 32, desc, stride, 32, n, hipMemcpyHostToDevice, h->stream));
  }
  const int r = vwd_add(v, h->vwd.io.as<uint8_t>(), n, node_id, n_keypoints_total, word_ids);
  if (r != SBM_OK) hipStreamSynchronize(h->stream);   // the enqueued copy reads the caller's rows
  return r;
}

int sbm_vwd_search_device(sbm_vwd* v, const void* d_desc, int n, void* d_knn, int sync) {
  if (!v || (n > 0 && (!d_desc || !d_knn))) return SBM_ERR_NULL;
  if (n < 0 || n > kMaxQueries) return SBM_ERR_SIZE;
  if (((uintptr_t)d_desc & 15) || ((uintptr_t)d_knn & 15)) return SBM_ERR_UNSUPPORTED;
  if (n == 0) return SBM_OK;
  sbm_handle* h = v->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  const int st = vwd_run(v, (const uint8_t*)d_desc, n, (int4*)d_knn, nullptr);
  if (st == SBM_OK && sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return st;
}

int sbm_vwd_fetch_words(sbm_vwd* v, size_t first, size_t count, uint8_t* rows) {
  if (!v || (count > 0 && !rows)) return SBM_ERR_NULL;
  sbm_handle* h = v->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  VwdCounters c;
  const int st = vwd_read_counters(v, &c);
  if (st != SBM_OK) return st;
  if (first > c.size || count > c.size - first) return SBM_ERR_SIZE;
  if (count) HIPCHK(h, hipMemcpy(rows, v->rows.as<uint8_t>() + first * 32, count * 32, hipMemcpyDeviceToHost));
  return SBM_OK;
}

int sbm_vwd_references(sbm_vwd* v, int word_id, int* nodes, int* counts, int cap, int* count) {
  if (!v || !count || (cap > 0 && (!nodes || !counts))) return SBM_ERR_NULL;
  if (word_id < 0 || (size_t)word_id >= v->refs.size() || cap < 0) return SBM_ERR_SIZE;
  const std::map<int, int>& r = v->refs[(size_t)word_id];
  *count = (int)r.size();
  if ((size_t)cap < r.size()) return SBM_ERR_SIZE;
  int k = 0;
  for (const auto& nc : r) {
    nodes[k] = nc.first;
    counts[k++] = nc.second;
  }
  return SBM_OK;
}

// computeLikelihood as written (Mapper.cpp:606-677) and detectLoopClosure's choice of the highest hypothesis (:568-573).
int sbm_vwd_likelihood(sbm_vwd* v, int node_id, const int* candidates, int n, int n_nodes, float* scores, int* best_id,
                       float* best_score) {
#pragma clang fp contract(off)
  if (!v || !best_id || !best_score || (n > 0 && (!candidates || !scores))) return SBM_ERR_NULL;
  if (n < 0 || n_nodes < 0) return SBM_ERR_SIZE;
  if (node_id < 1) return SBM_ERR_UNSUPPORTED;
  const auto self = v->nodes.find(node_id);
  if (self == v->nodes.end()) return SBM_ERR_SIZE;
  try {
    std::map<int, float> likelihood;
    for (int i = 0; i < n; i++) likelihood.insert(likelihood.end(), std::make_pair(candidates[i], 0.0f));
    std::vector<int> word_ids(self->second.words);   // the multimap's keys: ascending, then distinct
    std::sort(word_ids.begin(), word_ids.end());
    word_ids.erase(std::unique(word_ids.begin(), word_ids.end()), word_ids.end());
    const float N = (float)n_nodes;
    if (N) {
      for (const int w : word_ids) {
        if (w <= 0) continue;
        const std::map<int, int>& refs = v->refs[(size_t)w];
        const float nw = (float)refs.size();
        const float logNnw = log10f(N / nw);
        if (!logNnw) continue;
        for (const auto& j : refs) {
          const auto it = likelihood.find(j.first);
          if (it == likelihood.end()) continue;
          const float nwi = (float)j.second;
          const auto nd = v->nodes.find(j.first);
          if (nd == v->nodes.end()) continue;
          const int ni = (int)nd->second.ni;
          it->second += (nwi * logNnw) / ni;
        }
      }
    }
    for (int i = 0; i < n; i++) scores[i] = likelihood[candidates[i]];
    std::pair<int, float> best(0, 0.0f);
    for (const auto& s : likelihood)
      if (s.first > 0 && s.second > best.second) best = s;
    *best_id = best.first;
    *best_score = best.second;
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  return SBM_OK;
}

// SensorData::limitKeypoints: the multimap <fabs(response), index> walked from its end, which among equal responses meets the
// later insertion (the higher index) first.
int sbm_vwd_limit_keypoints(const float* responses, int n, int max, uint8_t* keep_flags) {
  if (n > 0 && (!responses || !keep_flags)) return SBM_ERR_NULL;
  if (n < 0) return SBM_ERR_SIZE;
  for (int i = 0; i < n; i++)
    if (std::isnan(responses[i])) return SBM_ERR_UNSUPPORTED;   // a multimap keyed on NaN has no order
  if (!(max > 0 && n > max)) {
    for (int i = 0; i < n; i++) keep_flags[i] = 1;
    return SBM_OK;
  }
  std::vector<int> order;
  try {
    order.resize((size_t)n);
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return fabsf(responses[a]) < fabsf(responses[b]); });
  memset(keep_flags, 0, (size_t)n);
  for (int k = 0; k < max; k++) keep_flags[order[(size_t)(n - 1 - k)]] = 1;
  return SBM_OK;
}

}  // extern "C"
