// sbm_occ_bt.hip -- the octomap binary stream (.bt) on the host: the writer of AbstractOccupancyOcTree::writeBinaryConst for a
// set of voxels, and the parser of readBinary that the loader (sbm_occ_load.hip) and the two inspection calls share; readHeader,
// which the .ot stream (sbm_occ_ot_host.hip) has too, and the file read of the read calls.
// Host only: no HIP header and no HIP call, so any C++17 compiler builds this file alone (tools/occupancy_load_sanitize.cpp does).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <new>
#include <string>

#include "sbm_occ.h"

namespace sbm {

// A leaf of the stream: its Morton code above bit 0, and in bit 0 whether toMaxLikelihood makes it occupied. Sorting the words
// sorts the codes.
// The inner node that covers leaves [lo, hi) (sorted, distinct codes) with `level` key bits still undecided (16 at the root): its
// two bytes, then its inner children depth first. A child whose range holds all 8^(level-1) codes below it, all of one kind, is
// what prune() leaves as one leaf of that kind. Returns the nodes written, this one included.
static size_t occ_write_node(const uint64_t* lo, const uint64_t* hi, int level, std::vector<uint8_t>& body) {
  const int shift = 3 * (level - 1) + 1;
  const uint64_t full = (uint64_t)1 << (shift - 1);   // 8^(level-1)
  const uint64_t* edge[9];
  edge[0] = lo;
  for (int c = 0; c < 8; c++) {
    const uint64_t* e = edge[c];
    while (e < hi && ((*e >> shift) & 7) == (uint64_t)c) e++;
    edge[c + 1] = e;
  }
  uint8_t byte[2] = {0, 0};
  bool inner[8];
  size_t nodes = 1;
  for (int c = 0; c < 8; c++) {
    const uint64_t cnt = (uint64_t)(edge[c + 1] - edge[c]);
    inner[c] = false;
    if (!cnt) continue;
    const uint64_t kind = *edge[c] & 1;
    inner[c] = cnt != full;
    for (const uint64_t* e = edge[c]; !inner[c] && e < edge[c + 1]; e++) inner[c] = (*e & 1) != kind;
    // bits (2c, 2c+1): 0,1 occupied leaf; 1,0 free leaf; 1,1 inner
    byte[c / 4] |= (uint8_t)((inner[c] ? 3 : kind ? 2 : 1) << (2 * (c % 4)));
    if (!inner[c]) nodes++;
  }
  body.push_back(byte[0]);
  body.push_back(byte[1]);
  for (int c = 0; c < 8; c++)
    if (inner[c]) nodes += occ_write_node(edge[c], edge[c + 1], level - 1, body);
  return nodes;
}

// The .bt file: the header of AbstractOccupancyOcTree::writeBinaryConst, `res` as operator<<(double) prints it (%g), then the body
int occ_write_file(const std::vector<uint8_t>& body, size_t nodes, double resolution, const char* path) {
  FILE* f = fopen(path, "wb");
  if (!f) return SBM_ERR_UNSUPPORTED;
  bool ok = fprintf(f,
                    "# Octomap OcTree binary file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\n"
                    "id OcTree\nsize %zu\nres %g\ndata\n",
                    nodes, resolution) > 0;
  ok = ok && (body.empty() || fwrite(body.data(), 1, body.size(), f) == body.size());
  ok = (fclose(f) == 0) && ok;
  return ok ? SBM_OK : SBM_ERR_UNSUPPORTED;
}

// What sbm_occ_write_binary* print for a resolution (%g), read back
double occ_printed_resolution(double resolution) {
  char text[64];
  snprintf(text, sizeof(text), "%g", resolution);
  return strtod(text, nullptr);
}

// ---- reading a .bt stream (include/sbm.h, "occupancy map: load a .bt stream") ------------------------------------------------
struct OccBtParse {
  sbm_occ_binary_header info;
  std::vector<OccBtLeaf>* leaves;   // null: count only
  bool bounds;                      // key_min / key_max are wanted
  const uint8_t *at, *end;
};

// AbstractOcTree::readHeader on bytes [*pos, n): tokens up to the line `data`. SBM_ERR_SIZE where the stream ends first or a
// number does not parse (octomap's stream fails there and its loop ends without `data`).
int occ_bt_header(const uint8_t* b, size_t n, size_t* pos, std::string* id, uint64_t* size, double* res) {
  size_t i = *pos;
  const auto space = [](uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
  const auto skip_line = [&] {
    while (i < n && b[i] != '\n') i++;
    if (i < n) i++;
  };
  const auto token = [&](std::string* t) {
    t->clear();
    while (i < n && space(b[i])) i++;
    while (i < n && !space(b[i])) t->push_back((char)b[i++]);
    return !t->empty();
  };
  std::string t;
  while (token(&t)) {
    if (t == "data") {
      skip_line();
      *pos = i;
      return SBM_OK;
    }
    if (t[0] == '#') {
      skip_line();
    } else if (t == "id") {
      if (!token(id)) return SBM_ERR_SIZE;
    } else if (t == "res" || t == "size") {
      while (i < n && space(b[i])) i++;
      char num[64];
      size_t len = 0;
      while (i + len < n && !space(b[i + len]) && len + 1 < sizeof(num)) num[len] = (char)b[i + len], len++;
      num[len] = 0;
      char* stop = num;
      if (t == "res") {
        *res = strtod(num, &stop);
      } else {
        if (num[0] < '0' || num[0] > '9') return SBM_ERR_SIZE;
        const unsigned long long v = strtoull(num, &stop, 10);
        if (v > 0xFFFFFFFFull) return SBM_ERR_SIZE;   // octomap's size is an unsigned
        *size = v;
      }
      if (stop == num) return SBM_ERR_SIZE;
      i += (size_t)(stop - num);   // what follows the number is the next token, as operator>> leaves it
    } else {
      skip_line();   // an unknown keyword: octomap warns and skips the line
    }
  }
  return SBM_ERR_SIZE;
}

// A leaf of the pruned tree: the node with Morton prefix `code` at `depth`
static int occ_bt_leaf(OccBtParse& p, uint64_t code, int depth, bool occupied) {
  sbm_occ_binary_header& o = p.info;
  const int level = 16 - depth;
  o.leaves++;
  o.leaves_at[depth]++;
  o.occupied += occupied ? 1 : 0;
  o.voxels += (uint64_t)1 << (3 * level);
  const uint64_t first = code << (3 * level);
  if (p.bounds) {
    const unsigned k[3] = {occ_unspread(first), occ_unspread(first >> 1), occ_unspread(first >> 2)};
    for (int a = 0; a < 3; a++) {
      o.key_min[a] = (uint16_t)std::min<unsigned>(o.key_min[a], k[a]);
      o.key_max[a] = (uint16_t)std::max<unsigned>(o.key_max[a], k[a] + (1u << level) - 1);
    }
  }
  if (p.leaves) p.leaves->push_back(first << 8 | (OccBtLeaf)depth << 1 | (occupied ? 1u : 0u));
  return SBM_OK;
}

// readBinaryNode of the node with Morton prefix `code` at `depth`, whose record is at p.at. Children in child order, depth first:
// the leaves arrive in Morton order.
static int occ_bt_node(OccBtParse& p, uint64_t code, int depth) {
  if (p.end - p.at < 2) return SBM_ERR_SIZE;   // the stream ends inside the tree
  const unsigned word = p.at[0] | (unsigned)p.at[1] << 8;
  p.at += 2;
  if (!word) return occ_bt_leaf(p, code, depth, true);   // a childless node keeps the clamp max readBinaryNode gave it
  for (int c = 0; c < 8; c++) {
    const unsigned kind = word >> (2 * c) & 3;
    if (!kind) continue;
    p.info.nodes++;
    int st;
    if (kind != 3) st = occ_bt_leaf(p, code << 3 | c, depth + 1, kind == 2);
    else if (depth + 1 >= 16) st = SBM_ERR_SIZE;             // a node below depth 16
    else st = occ_bt_node(p, code << 3 | c, depth + 1);
    if (st != SBM_OK) return st;
  }
  return SBM_OK;
}

// AbstractOccupancyOcTree::readBinary on n bytes -> the header's counts and, with `leaves`, the leaves in stream order
int occ_bt_parse(const uint8_t* b, size_t n, sbm_occ_binary_header* info, std::vector<OccBtLeaf>* leaves, bool bounds) {
  static const char magic[] = "# Octomap OcTree binary file";
  OccBtParse p;
  memset(&p.info, 0, sizeof(p.info));
  for (int a = 0; a < 3; a++) p.info.key_min[a] = 0xFFFF;
  p.leaves = leaves;
  p.bounds = bounds && info != nullptr;
  int st = SBM_OK;
  size_t pos = 0;
  std::string id;
  try {
    if (n < sizeof(magic) - 1 || memcmp(b, magic, sizeof(magic) - 1) != 0) {
      st = SBM_ERR_UNSUPPORTED;   // the legacy header, or no .bt at all
    } else {
      while (pos < n && b[pos] != '\n') pos++;   // std::getline
      if (pos < n) pos++;
      st = occ_bt_header(b, n, &pos, &id, &p.info.size, &p.info.resolution);
    }
    if (st == SBM_OK && id != "OcTree" && id != "1") st = SBM_ERR_UNSUPPORTED;   // "1" is the id octomap itself renames
    if (st == SBM_OK && !(p.info.resolution > 0.)) st = SBM_ERR_SIZE;
    if (st == SBM_OK && p.info.size > 0) {
      if (leaves) leaves->reserve((size_t)std::min<uint64_t>(p.info.size, 4 * (uint64_t)(n - pos)));   // a record has 8 children at most
      p.at = b + pos;
      p.end = b + n;
      p.info.nodes = 1;
      st = occ_bt_node(p, 0, 0);
    }
  } catch (const std::bad_alloc&) {
    st = SBM_ERR_NOMEM;
  }
  if (st == SBM_OK && p.info.nodes != p.info.size) st = SBM_ERR_SIZE;   // calcNumNodes() against the header
  if (info) *info = p.info;
  return st;
}

// A whole file into memory: what the two read calls share
int occ_read_file(const char* path, std::vector<uint8_t>* data) {
  FILE* f = fopen(path, "rb");
  if (!f) return SBM_ERR_UNSUPPORTED;
  bool ok = true;
  try {
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) data->insert(data->end(), chunk, chunk + got);
    ok = !ferror(f);
  } catch (const std::bad_alloc&) {
    fclose(f);
    return SBM_ERR_NOMEM;
  }
  fclose(f);
  return ok ? SBM_OK : SBM_ERR_UNSUPPORTED;
}

// A voxel as the writer's leaf word: occ_code masks each field of the packed key to its 16 bits
static uint64_t occ_leaf_word(uint64_t key, bool occupied) { return occ_code(key >> 32, key >> 16, key) << 1 | (occupied ? 1 : 0); }

// AbstractOccupancyOcTree::writeBinaryConst of n voxels: occupied all of them and free to repeat (logodds null), or each what its
// value says against `thres` (isNodeOccupied) and one value per voxel
static int occ_write_keys(const uint64_t* keys, const float* logodds, size_t n, double resolution, float thres, const char* path) {
  if (!path || (n > 0 && !keys)) return SBM_ERR_NULL;
  if (!std::isfinite(resolution) || !(resolution > 0.) || std::isnan(thres)) return SBM_ERR_SIZE;
  std::vector<uint64_t> leaf;
  std::vector<uint8_t> body;
  size_t nodes = 0;
  try {
    leaf.reserve(n);
    for (size_t i = 0; i < n; i++) {
      if (keys[i] >> 48 || (logodds && std::isnan(logodds[i]))) return SBM_ERR_SIZE;
      leaf.push_back(occ_leaf_word(keys[i], !logodds || logodds[i] >= thres));
    }
    std::sort(leaf.begin(), leaf.end());
    if (!logodds) leaf.erase(std::unique(leaf.begin(), leaf.end()), leaf.end());
    for (size_t i = 1; i < leaf.size(); i++)
      if (leaf[i] >> 1 == leaf[i - 1] >> 1) return SBM_ERR_SIZE;   // one value per voxel
    if (!leaf.empty()) nodes = occ_write_node(leaf.data(), leaf.data() + leaf.size(), 16, body);
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  return occ_write_file(body, nodes, resolution, path);
}

}  // namespace sbm
using namespace sbm;

extern "C" {
int sbm_occ_write_binary(const uint64_t* keys, size_t n, double resolution, const char* path) {
  return occ_write_keys(keys, nullptr, n, resolution, 0.0f, path);
}

int sbm_occ_write_binary_logodds(const uint64_t* keys, const float* logodds, size_t n, double resolution, float occupancy_thres_log,
                                 const char* path) {
  if (n > 0 && !logodds) return SBM_ERR_NULL;
  return occ_write_keys(keys, logodds, n, resolution, occupancy_thres_log, path);
}

int sbm_occ_binary_info(const void* bytes, size_t n, sbm_occ_binary_header* out) {
  if (!out || (n > 0 && !bytes)) return SBM_ERR_NULL;
  return occ_bt_parse((const uint8_t*)bytes, n, out, nullptr);
}

int sbm_occ_binary_leaves(const void* bytes, size_t n, uint64_t* first_key, int32_t* depth, uint8_t* occupied, size_t cap, size_t* count) {
  if (!count || (n > 0 && !bytes) || (cap > 0 && (!first_key || !depth || !occupied))) return SBM_ERR_NULL;
  std::vector<OccBtLeaf> leaves;
  const int st = occ_bt_parse((const uint8_t*)bytes, n, nullptr, &leaves);
  if (st != SBM_OK) return st;
  *count = leaves.size();
  if (leaves.size() > cap) return SBM_ERR_SIZE;
  for (size_t i = 0; i < leaves.size(); i++) {
    first_key[i] = occ_key_of_code(occ_bt_code(leaves[i]));
    depth[i] = occ_bt_depth(leaves[i]);
    occupied[i] = (uint8_t)(leaves[i] & 1);
  }
  return SBM_OK;
}
}  // extern "C"
