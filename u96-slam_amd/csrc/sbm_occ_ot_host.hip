// sbm_occ_ot_host.hip -- the .ot stream on the host (include/sbm.h, "occupancy map: the .ot format"): its header, its file, and
// the one-pass parser of AbstractOcTree::read (recursion depth at most 16) that sbm_occ_ot_info / sbm_occ_ot_leaves run and the
// loader (sbm_occ_ot.hip) can take instead of its device parse.
// Host only: no HIP header and no HIP call, so any C++17 compiler builds this file and sbm_occ_bt.hip alone
// (tools/occupancy_ot_sanitize.cpp does).
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <new>
#include <string>

#include "sbm_occ.h"

namespace sbm {

// AbstractOcTree::write: the header, `res` printed as the .bt writers print it, then five bytes per node
int occ_ot_write_file(const std::vector<uint8_t>& body, size_t nodes, double resolution, const char* path, const char* id) {
  FILE* f = fopen(path, "wb");
  if (!f) return SBM_ERR_UNSUPPORTED;
  bool ok = fprintf(f,
                    "# Octomap OcTree file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\n"
                    "id %s\nsize %zu\nres %g\ndata\n",
                    id, nodes, resolution) > 0;
  ok = ok && (body.empty() || fwrite(body.data(), 1, body.size(), f) == body.size());
  ok = (fclose(f) == 0) && ok;
  return ok ? SBM_OK : SBM_ERR_UNSUPPORTED;
}

// AbstractOcTree::read up to the body: the first line, readHeader's tokens, the id, res, and that the body holds `size` records.
// `want_res` (> 0): the map's printed resolution, which the file's must equal.
int occ_ot_head(const uint8_t* b, size_t n, double want_res, sbm_occ_ot_header* info, size_t* body, bool stamped) {
  static const char magic[] = "# Octomap OcTree file";
  memset(info, 0, sizeof(*info));
  for (int a = 0; a < 3; a++) info->key_min[a] = 0xFFFF;
  if (n < sizeof(magic) - 1 || memcmp(b, magic, sizeof(magic) - 1) != 0) return SBM_ERR_UNSUPPORTED;   // a .bt, or no octomap file
  size_t pos = 0;
  while (pos < n && b[pos] != '\n') pos++;   // std::getline
  if (pos < n) pos++;
  std::string id;
  const int st = occ_bt_header(b, n, &pos, &id, &info->size, &info->resolution);
  if (st != SBM_OK) return st;
  if (stamped ? id != "OcTreeStamped" : (id != "OcTree" && id != "1")) return SBM_ERR_UNSUPPORTED;   // the one difference of the stamped stream
  if (!(info->resolution > 0.)) return SBM_ERR_SIZE;
  if (want_res > 0. && info->resolution != want_res) return SBM_ERR_SIZE;
  if (info->size > (n - pos) / 5) return SBM_ERR_SIZE;
  *body = pos;
  return SBM_OK;
}

struct OccOtParse {
  sbm_occ_ot_header* info;
  std::vector<OccBtLeaf>* words;     // null: count only
  std::vector<uint32_t>* values;
  const uint8_t* rec;
  uint64_t at;                       // records read
  bool bounds, bad_value, any;
};

// readNodesRecurs of the node with Morton prefix `code` at `depth`: its record, then its children's in ascending child index
static int occ_ot_node(OccOtParse& p, uint64_t code, int depth) {
  sbm_occ_ot_header& o = *p.info;
  if (p.at >= o.size) return SBM_ERR_SIZE;   // still open after `size` records
  const uint8_t* r = p.rec + 5 * p.at++;
  const uint32_t value = r[0] | (uint32_t)r[1] << 8 | (uint32_t)r[2] << 16 | (uint32_t)r[3] << 24;
  const unsigned mask = r[4];
  o.nodes = p.at;
  if (!mask) {
    const int level = 16 - depth;
    float v;
    memcpy(&v, &value, 4);
    if (!std::isfinite(v)) {
      p.bad_value = true;
    } else {
      o.value_min = p.any ? std::min(o.value_min, v) : v;
      o.value_max = p.any ? std::max(o.value_max, v) : v;
      p.any = true;
    }
    o.leaves++;
    o.leaves_at[depth]++;
    o.voxels += (uint64_t)1 << (3 * level);
    const uint64_t first = code << (3 * level);
    if (p.bounds) {
      const unsigned k[3] = {occ_unspread(first), occ_unspread(first >> 1), occ_unspread(first >> 2)};
      for (int a = 0; a < 3; a++) {
        o.key_min[a] = (uint16_t)std::min<unsigned>(o.key_min[a], k[a]);
        o.key_max[a] = (uint16_t)std::max<unsigned>(o.key_max[a], k[a] + (1u << level) - 1);
      }
    }
    if (p.words) {
      p.words->push_back(first << 8 | (OccBtLeaf)depth << 1);
      p.values->push_back(value);
    }
    return SBM_OK;
  }
  if (depth >= 16) return SBM_ERR_SIZE;      // a child bit at depth 16
  for (int c = 0; c < 8; c++)
    if (mask >> c & 1) {
      const int st = occ_ot_node(p, code << 3 | c, depth + 1);
      if (st != SBM_OK) return st;
    }
  return SBM_OK;
}

// The body after occ_ot_head accepted the stream: the shape of the tree over the first `size` records, then the leaf values.
// The cubes of a tree are disjoint, so `voxels` is at most 2^48.
int occ_ot_parse(const uint8_t* b, size_t n, double want_res, sbm_occ_ot_header* info, std::vector<OccBtLeaf>* words,
                 std::vector<uint32_t>* values, bool bounds, bool stamped) {
  size_t body = 0;
  int st = occ_ot_head(b, n, want_res, info, &body, stamped);
  if (st != SBM_OK || !info->size) return st;
  OccOtParse p;
  p.info = info;
  p.words = words;
  p.values = values;
  p.rec = b + body;
  p.at = 0;
  p.bounds = bounds;
  p.bad_value = p.any = false;
  try {
    if (words) {
      words->reserve((size_t)info->size);
      values->reserve((size_t)info->size);
    }
    st = occ_ot_node(p, 0, 0);
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  if (st == SBM_OK && info->nodes != info->size) st = SBM_ERR_SIZE;   // the tree completes before `size` records
  if (st == SBM_OK && p.bad_value) st = SBM_ERR_UNSUPPORTED;
  return st;
}

}  // namespace sbm
using namespace sbm;

extern "C" {
int sbm_occ_ot_info(const void* bytes, size_t n, sbm_occ_ot_header* out) {
  if (!out || (n > 0 && !bytes)) return SBM_ERR_NULL;
  return occ_ot_parse((const uint8_t*)bytes, n, 0., out, nullptr, nullptr, true);
}

static int occ_ot_leaves_of(const void* bytes, size_t n, uint64_t* first_key, int32_t* depth, float* value, size_t cap, size_t* count, bool stamped) {
  if (!count || (n > 0 && !bytes) || (cap > 0 && (!first_key || !depth || !value))) return SBM_ERR_NULL;
  sbm_occ_ot_header info;
  std::vector<OccBtLeaf> words;
  std::vector<uint32_t> values;
  const int st = occ_ot_parse((const uint8_t*)bytes, n, 0., &info, &words, &values, false, stamped);
  if (st != SBM_OK) return st;
  *count = words.size();
  if (words.size() > cap) return SBM_ERR_SIZE;
  for (size_t i = 0; i < words.size(); i++) {
    first_key[i] = occ_key_of_code(occ_bt_code(words[i]));
    depth[i] = occ_bt_depth(words[i]);
    memcpy(&value[i], &values[i], 4);
  }
  return SBM_OK;
}
int sbm_occ_ot_leaves(const void* bytes, size_t n, uint64_t* first_key, int32_t* depth, float* value, size_t cap, size_t* count) {
  return occ_ot_leaves_of(bytes, n, first_key, depth, value, cap, count, false);
}
// the `id OcTreeStamped` stream: the plain records (OcTreeNodeStamped writes no stamp), so the plain parser with the other id test
int sbm_occ_stamp_ot_info(const void* bytes, size_t n, sbm_occ_ot_header* out) {
  if (!out || (n > 0 && !bytes)) return SBM_ERR_NULL;
  return occ_ot_parse((const uint8_t*)bytes, n, 0., out, nullptr, nullptr, true, true);
}
int sbm_occ_stamp_ot_leaves(const void* bytes, size_t n, uint64_t* first_key, int32_t* depth, float* value, size_t cap, size_t* count) {
  return occ_ot_leaves_of(bytes, n, first_key, depth, value, cap, count, true);
}
}  // extern "C"
