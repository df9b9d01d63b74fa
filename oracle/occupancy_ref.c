// occupancy_ref.c -- sequential CPU restatement of the reference's buildOccupancyGridMap (src/slam/src/core/main.cpp:495-561)
// as include/sbm.h states it ("occupancy map: buildOccupancyGridMap"), and of the octomap binary stream that
// OcTree::writeBinary produces for a tree of occupied leaves. TEST INFRASTRUCTURE ONLY: never linked into the engine, and
// its writer (a pointer octree with an explicit prune) shares nothing with the library's (one pass over Morton-sorted keys).
// Built by oracle/Makefile with -O2 -ffp-contract=off: every float / double operation below is the one the C++ source performs.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct {   // sbm_stereo_model
  double fx_l, fy_l, cx_l, cy_l, Tx_l;
  double fx_r, fy_r, cx_r, Tx_r;
  float local[12];
  int32_t has_local;
} occ_model;

typedef struct {   // sbm_occ_params
  double resolution;
  float range_max;
  int32_t tree_depth;
} occ_params;

#define OCC_EMPTY 0xFFFFFFFFFFFFFFFFull
#define OCC_GATE 1   // the range gate keeps the point
#define OCC_KEY 2    // coordToKeyChecked accepts it

// Stereo.cpp:157-182; returns 0 where the reference skips the pixel (disparity <= 0 or a coordinate that is not finite)
static int project(float px, float py, float disp, const occ_model* m, float* p) {
  if (!(disp > 0.0f)) return 0;
  const float c = (float)(m->cx_r - m->cx_l);
  const float dc = disp + c;
  const float Wx = (float)((m->Tx_l / m->fx_l - m->Tx_r / m->fx_r) / (double)dc);
  const float Wy = (float)((m->Tx_l / m->fy_l - m->Tx_r / m->fy_r) / (double)dc);
  p[0] = (float)(((double)px - m->cx_l) * (double)Wx);
  p[1] = (float)(((double)py - m->cy_l) * (double)Wy);
  p[2] = (float)(m->fx_l * (double)Wx);
  return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}

// Stereo.cpp:189-198
static void transform(float* p, const float* t) {
  const float x = p[0], y = p[1], z = p[2];
  p[0] = t[0] * x + t[1] * y + t[2] * z + t[3];
  p[1] = t[4] * x + t[5] * y + t[6] * z + t[7];
  p[2] = t[8] * x + t[9] * y + t[10] * z + t[11];
}

void occ_ref_reproject(const int16_t* disp, int w, int h, int scale, const occ_model* m, int apply_local, float* xyz) {
  for (int r = 0; r < h; r++)
    for (int c = 0; c < w; c++) {
      float* o = xyz + 3 * ((size_t)r * w + c);
      const float d = (float)(disp[(size_t)r * w + c] / 16.0f);
      float p[3];
      if (d > 0 && project((float)(c * scale), (float)(r * scale), d, m, p)) {
        if (apply_local && m->has_local) transform(p, m->local);
        o[0] = p[0], o[1] = p[1], o[2] = p[2];
      } else {
        o[0] = o[1] = o[2] = NAN;
      }
    }
}

// main.cpp:529-539 of one plane: the world point of every pixel, NaN where the pixel is skipped
void occ_ref_world(const int16_t* disp, int w, int h, int scale, const occ_model* m, const float* pose, float* xyz) {
  for (int r = 0; r < h; r++)
    for (int c = 0; c < w; c++) {
      float* o = xyz + 3 * ((size_t)r * w + c);
      const float d = (float)(disp[(size_t)r * w + c] / 16.0f);
      float p[3];
      if (d > 0 && project((float)(c * scale), (float)(r * scale), d, m, p)) {
        if (m->has_local) transform(p, m->local);
        transform(p, pose);
        o[0] = p[0], o[1] = p[1], o[2] = p[2];
      } else {
        o[0] = o[1] = o[2] = NAN;
      }
    }
}

// OcTreeBaseImpl.hxx:310-321 on one axis; what x86's cvttsd2si gives for a double that no int holds is INT_MIN, which the
// range test then rejects, so "does not fit" and "not finite" both reject
static int axis_key(double factor, double coord, uint16_t* k) {
  const double f = floor(factor * coord);
  if (!(f >= -2147483648.0 && f <= 2147483647.0)) return 0;
  const long long s = (long long)f + 32768;
  if (s < 0 || s >= 65536) return 0;
  *k = (uint16_t)s;
  return 1;
}

// main.cpp:541-548 on one world point: *norm = Vector3::norm() of the offset; the returned bits say which tests passed;
// key[] holds the accepted axes' keys
int occ_ref_point(const float* pt, const float* origin, const occ_params* prm, double* norm, uint16_t* key) {
  const float range_max_sqrd = prm->range_max * prm->range_max;
  const float vx = pt[0] - origin[0], vy = pt[1] - origin[1], vz = pt[2] - origin[2];
  const float nsq = vx * vx + vy * vy + vz * vz;      // Vector3::norm_sq: a float expression returned as double
  const double n = sqrt((double)nsq);
  if (norm) *norm = n;
  int bits = n <= (double)range_max_sqrd ? OCC_GATE : 0;   // the norm against the SQUARED range, as the source has it
  const double factor = 1. / prm->resolution;
  int ok = 1;
  for (int a = 0; a < 3; a++) {
    key[a] = 0;
    ok &= axis_key(factor, (double)pt[a], &key[a]);
  }
  return bits | (ok ? OCC_KEY : 0);
}

// per pixel of n planes (poses: n * 12 floats) the packed key k0 << 32 | k1 << 16 | k2, or OCC_EMPTY
void occ_ref_keys(int n, const int16_t* disp, int w, int h, int scale, const occ_model* m, const float* poses,
                  const occ_params* prm, uint64_t* keys) {
  for (int p = 0; p < n; p++) {
    const float* pose = poses + 12 * p;
    const float origin[3] = {pose[3], pose[7], pose[11]};
    for (int r = 0; r < h; r++)
      for (int c = 0; c < w; c++) {
        const size_t i = ((size_t)p * h + r) * w + c;
        keys[i] = OCC_EMPTY;
        const float d = (float)(disp[i] / 16.0f);
        float pt[3];
        if (!(d > 0) || !project((float)(c * scale), (float)(r * scale), d, m, pt)) continue;
        if (m->has_local) transform(pt, m->local);
        transform(pt, pose);
        uint16_t k[3];
        if (occ_ref_point(pt, origin, prm, NULL, k) != (OCC_GATE | OCC_KEY)) continue;
        keys[i] = (uint64_t)k[0] << 32 | (uint64_t)k[1] << 16 | k[2];
      }
  }
}

// ---- the .bt stream: a pointer octree, updateNode per key, prune, writeBinary ---------------------------------------------
typedef struct Node {
  struct Node* child[8];
} Node;

static int has_children(const Node* n) {
  for (int i = 0; i < 8; i++)
    if (n->child[i]) return 1;
  return 0;
}

static void free_tree(Node* n) {
  if (!n) return;
  for (int i = 0; i < 8; i++) free_tree(n->child[i]);
  free(n);
}

// OcTreeBaseImpl::pruneNode, bottom up: eight childless children (all occupied here) collapse into their parent
static void prune(Node* n) {
  int full = 1;
  for (int i = 0; i < 8; i++) {
    if (!n->child[i]) { full = 0; continue; }
    prune(n->child[i]);
    if (has_children(n->child[i])) full = 0;
  }
  if (!full) return;
  for (int i = 0; i < 8; i++) {
    free(n->child[i]);
    n->child[i] = NULL;
  }
}

static void count(const Node* n, unsigned* nodes, unsigned* leafs) {
  ++*nodes;
  if (!has_children(n)) { ++*leafs; return; }
  for (int i = 0; i < 8; i++)
    if (n->child[i]) count(n->child[i], nodes, leafs);
}

typedef struct { uint8_t* p; size_t n, cap; } Buf;

static void put(Buf* b, const void* src, size_t n) {
  if (b->n + n <= b->cap) memcpy(b->p + b->n, src, n);
  b->n += n;
}

// OccupancyOcTreeBase::writeBinaryNode: 2 bits per child (01 occupied leaf, 11 inner, 00 unknown), children 0-3 then 4-7,
// then the inner children in order
static void write_node(Buf* b, const Node* n) {
  uint8_t byte[2] = {0, 0};
  for (int i = 0; i < 8; i++) {
    if (!n->child[i]) continue;
    const int bits = has_children(n->child[i]) ? 3 : 2;   // bit 2i, bit 2i+1: (1,1) inner, (0,1) occupied
    byte[i / 4] |= (uint8_t)(bits << (2 * (i % 4)));
  }
  put(b, byte, 2);
  for (int i = 0; i < 8; i++)
    if (n->child[i] && has_children(n->child[i])) write_node(b, n->child[i]);
}

// Bytes of writeBinary for a tree that holds exactly these packed keys as occupied leaves; returns the length (the stream is
// complete only when it is <= cap); *nodes = size() after the prune, *leafs = getNumLeafNodes() after it.
size_t occ_ref_write_binary(const uint64_t* keys, size_t n, double resolution, uint8_t* out, size_t cap, unsigned* nodes,
                            unsigned* leafs) {
  Node* root = NULL;
  for (size_t i = 0; i < n; i++) {
    const unsigned k[3] = {(unsigned)(keys[i] >> 32) & 0xFFFF, (unsigned)(keys[i] >> 16) & 0xFFFF, (unsigned)keys[i] & 0xFFFF};
    if (!root) root = calloc(1, sizeof(Node));
    Node* cur = root;
    for (int bit = 15; bit >= 0; bit--) {   // computeChildIdx: x -> 1, y -> 2, z -> 4
      const int idx = ((k[0] >> bit) & 1) | ((k[1] >> bit) & 1) << 1 | ((k[2] >> bit) & 1) << 2;
      if (!cur->child[idx]) cur->child[idx] = calloc(1, sizeof(Node));
      cur = cur->child[idx];
    }
  }
  unsigned nn = 0, nl = 0;
  if (root) {
    for (int i = 0; i < 8; i++)           // prune() never collapses the root's children into the root
      if (root->child[i]) prune(root->child[i]);
    count(root, &nn, &nl);
  }
  if (nodes) *nodes = nn;
  if (leafs) *leafs = nl;
  Buf b = {out, 0, cap};
  char head[256];
  const int len = snprintf(head, sizeof(head),
                           "# Octomap OcTree binary file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\n"
                           "id OcTree\nsize %u\nres %g\ndata\n",
                           nn, resolution);
  put(&b, head, (size_t)len);
  if (root) write_node(&b, root);
  free_tree(root);
  return b.n;
}
